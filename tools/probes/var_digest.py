#!/usr/bin/env python3
"""Digests of everything the varying scans and the smoothing plan compute, for comparing two builds of the library bit for bit.

    RECFILTER_AMD_LIB=/path/to/other/librecfilter_amd.so python tools/probes/var_digest.py > other.txt
    python tools/probes/var_digest.py > built.txt && cmp other.txt built.txt

With fixed seeds, on small shapes at which the indexing can still go wrong -- (64, 64): one tile each way; (65, 68) and (130, 132):
a partial last tile, more than two tiles, H != W -- and 1 and 3 planes, one line per case:  <case name> <sha256 of every output
plane's bytes>.  The cases: VarPlan.execute / execute_power and backward / backward_power (no weight gradients, all of them,
[None, plane], in place) for pair stages, -x +x, +y alone and +x -x on two weight planes; the two distance entry points; SmoothPlan
with K = 1 and 3 for f32 and uint8 images and guides, in place, both backward forms, and batch = 1 and 3.  Every *_timed twin must
give the digest of its untimed call (else the probe exits with status 1); its line ends in names:<k>, the number of the name list
it reports, and the distinct lists are printed at the end (names:<k> <names>), so two outputs compare the launch lists as well.
No time is printed: the output of one build is the same from run to run."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = [(64, 64), (65, 68), (130, 132)]
SCAN_LISTS = {      # name: (scans, weight planes)
    "+x-x+y-y": ([(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)], 2),
    "-x+x": ([(0, False, 0), (0, True, 0)], 1),
    "+y": ([(1, True, 0)], 1),
    "+x-x.two": ([(0, True, 0), (0, False, 1)], 2),
}
SIGMA_S, SIGMA_R = 12.0, 0.4
mismatches = 0


def digest(*groups):
    h = hashlib.sha256()
    for group in groups:
        for t in ([group] if hasattr(group, "dim") or group is None else group):
            h.update(b"none" if t is None else t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


name_lists = {}      # the distinct name lists of the timed calls, numbered as they are first met


def report(case, plain, timed=None, times=None):
    """one line for the untimed call; its timed twin must agree, and adds the number of the name list it reports"""
    global mismatches
    if timed is None:
        print(f"{case} {plain}")
        return
    if timed != plain:
        mismatches += 1
        print(f"{case} TIMED TWIN DIFFERS {timed}")
    k = name_lists.setdefault(",".join(name for name, _ in times), len(name_lists))
    print(f"{case} {plain} names:{k}")


def var_cases(rand, H, W, P):
    import recfilter_amd as rfa
    for tag, (scans, K) in SCAN_LISTS.items():
        case = f"var {H}x{W} p{P} {tag}"
        ins = [rand(H, W) for _ in range(P)]
        weights = [0.05 + 0.9 * rand(H, W) for _ in range(K)]
        exponents = [1.0 + 3.0 * rand(H, W) for _ in range(K)]
        bases = [0.8, 0.6][:K]
        grads = [rand(H, W) * 2 - 1 for _ in range(P)]
        with rfa.VarPlan((H, W), scans, planes=P, n_weights=K) as plan:
            outs, times = plan.execute_timed(ins, weights)
            report(f"{case} execute", digest(plan.execute(ins, weights)), digest(outs), times)
            outs, times = plan.execute_power_timed(ins, exponents, bases)
            report(f"{case} execute_power", digest(plan.execute_power(ins, exponents, bases)), digest(outs), times)
            forms = (("backward", plan.backward, plan.backward_timed, (weights,)),
                     ("backward_power", plan.backward_power, plan.backward_power_timed, (exponents, bases)))
            for form, run, run_timed, w in forms:
                zeros = lambda: [t.new_zeros(t.shape) for t in w[0]]      # noqa: E731
                variants = [("image", lambda: (None, *w, [g.clone() for g in grads], None, None)),
                            ("all", lambda: (ins, *w, [g.clone() for g in grads], None, zeros())),
                            ("inplace", lambda: (ins, *w, *([g.clone() for g in grads],) * 2, zeros()))]
                if K == 2:
                    variants.append(("none+plane", lambda: (ins, *w, [g.clone() for g in grads], None, [None, zeros()[1]])))
                for variant, arguments in variants:
                    gi, gw = run(*arguments())
                    gi_t, gw_t, times = run_timed(*arguments())
                    report(f"{case} {form} {variant}", digest(gi, gw or []), digest(gi_t, gw_t or []), times)


def distance_cases(rand, H, W, C):
    import torch
    import recfilter_amd as rfa
    case = f"distances {H}x{W} c{C}"
    guide = rand(C, H, W)
    report(f"{case} f32", digest(rfa.domain_transform_distances(guide, SIGMA_S, SIGMA_R)))
    report(f"{case} uint8", digest(rfa.domain_transform_distances((guide * 255).to(torch.uint8), SIGMA_S, SIGMA_R)))
    gdx, gdy, held = rand(H, W) * 2 - 1, rand(H, W) * 2 - 1, rand(C, H, W)
    report(f"{case} backward stored", digest(rfa.domain_transform_distances_backward(guide, SIGMA_S, SIGMA_R, gdx, gdy)))
    report(f"{case} backward accumulate", digest(rfa.domain_transform_distances_backward(guide, SIGMA_S, SIGMA_R, gdx, gdy, held, accumulate=True)))


def smooth_cases(rand, H, W, P, K):
    import torch
    import recfilter_amd as rfa
    u8, f32 = torch.uint8, torch.float32
    make = lambda **kw: rfa.SmoothPlan((H, W), planes=P, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R, **kw)      # noqa: E731
    case = f"smooth {H}x{W} p{P} K{K}"
    image, guide, grad = rand(P, H, W), rand(2, H, W), rand(P, H, W) * 2 - 1
    image8, guide8 = (image * 255).to(u8), (guide * 255).to(u8)

    def forward(tag, plan, img, g, in_place=False):
        first, second = (img.clone(), img.clone()) if in_place else (img, img)
        out, times = plan.execute_timed(second, g, second if in_place else None)
        report(f"{case} {tag}", digest(plan.execute(first, g, first if in_place else None)), digest(out), times)

    def backward(tag, plan, img, g, go, edges, in_place=False):
        first = go.clone()
        gi, gg = plan.backward(img, g, first, first if in_place else None, None, edges=edges)
        second = go.clone()
        gi_t, gg_t, times = plan.backward_timed(img, g, second, second if in_place else None, None, edges=edges)
        report(f"{case} {tag} edges={int(edges)}" + (" inplace" if in_place else ""), digest(gi, gg), digest(gi_t, gg_t), times)
    with make() as plan:
        forward("self f32", plan, image, None)
        forward("self f32 inplace", plan, image, None, in_place=True)
        for edges in (False, True):
            backward("self f32 backward", plan, image, None, grad, edges)
            backward("self f32 backward", plan, image, None, grad, edges, in_place=True)
    with make(guide_planes=2) as plan:
        forward("guide f32", plan, image, guide)
        for edges in (False, True):
            backward("guide f32 backward", plan, image, guide, grad, edges)
    with make(image_dtype=u8) as plan:
        forward("self uint8", plan, image8, None)
    with make(guide_planes=2, guide_dtype=u8) as plan:
        forward("guide uint8", plan, image, guide8)
        backward("guide uint8 backward", plan, None, guide8, grad, False)
    for N in (1, 3):
        images, guides, grads = rand(N, P, H, W), rand(N, 2, H, W), rand(N, P, H, W) * 2 - 1
        with make(batch=N) as plan:
            forward(f"batch{N} self f32", plan, images, None)
            for edges in (False, True):
                backward(f"batch{N} self f32 backward", plan, images, None, grads, edges)
        with make(batch=N, guide_planes=2) as plan:
            forward(f"batch{N} guide f32", plan, images, guides)
            for edges in (False, True):
                backward(f"batch{N} guide f32 backward", plan, images, guides, grads, edges)
        with make(batch=N, image_dtype=u8) as plan:
            forward(f"batch{N} self uint8", plan, (images * 255).to(u8), None)


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit("var_digest: needs a GPU")
    gen = torch.Generator().manual_seed(21)      # on the host: the same numbers whatever the device's generator does
    rand = lambda *shape: torch.rand(shape, generator=gen).cuda()      # noqa: E731
    for H, W in SHAPES:
        for P in (1, 3):
            var_cases(rand, H, W, P)
            distance_cases(rand, H, W, P)
            for K in (1, 3):
                smooth_cases(rand, H, W, P, K)
    torch.cuda.synchronize()
    for names, k in name_lists.items():
        print(f"names:{k} {names}")
    sys.exit(1 if mismatches else 0)


if __name__ == "__main__":
    main()
