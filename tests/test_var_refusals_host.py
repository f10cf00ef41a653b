"""What the host layer of the varying scans refuses, message by message and in order, on a machine without a GPU: the three
plan descriptions (image, signal, volume), the three smoothing descriptions (image, batch, volume) and the four distance calls.

Every entry point has a table of faults in the order its validator decides them.  A case is either one fault alone or two
consecutive faults at once, where the earlier one must win; a few cases that are not consecutive are listed beside them (the two
orders of `accumulate` against the extents, a fault in scan 0 against an earlier kind of fault in scan 1).  The descriptions are
host-only and the distance calls take made-up addresses that are never dereferenced: every case is a refusal, so no kernel is
launched and nothing of HIP is called.

tests/golden/var_refusals.json holds (case id, status, full message) for every case, and the test asserts exact equality.  The
fixture records what the library answered BEFORE the validators and the distance runners were merged into one each
(`python tests/test_var_refusals_host.py --record` on that build); it is the reference of that merge and is not regenerated from
the code it checks.  A new refusal gets a new case, recorded by itself."""
import ctypes
import functools
import json
import os
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recfilter_amd import capi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "var_refusals.json")
HOST = capi.RF_DEVICE_HOST_ONLY
MAXE = 1 << 21                    # the highest extent of the varying scans
A, B, C, D, E, G = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x700000      # 16-byte aligned, never dereferenced
EXCLUSIVE = "exclusive"           # with_next: the two faults cannot hold at once (one field, two disjoint ranges)


def fault(name, single, with_next=None):
    """one refusal: the overrides that provoke it alone, and (where merging them with the next fault's would not give both faults)
    the overrides that give this fault and the next one at once"""
    return name, single, with_next


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def arr(values):
    return None if values is None else (ctypes.c_void_p * max(len(values), 1))(*values)


def answer(status, handle=None, destroy=None):
    text = capi.lib().rf_last_error_string().decode()
    if handle is not None and handle.value:
        getattr(capi.lib(), destroy)(handle)
    return int(status), text


def scan_array(f):
    """(the array kept alive, pointer or null, n_scans) of f["scans"], a list of (dim, causal, weights) or None for a null pointer"""
    scans = f["scans"]
    n = f["n_scans"] if f["n_scans"] is not None else len(scans) if scans is not None else 2
    if scans is None:
        return None, None, n
    keep = (capi.VarScanDesc * max(len(scans), 1))()
    for i, (dim, causal, weights) in enumerate(scans):
        keep[i].dim, keep[i].causal, keep[i].weights = dim, causal, weights
    return keep, ctypes.cast(keep, ctypes.POINTER(capi.VarScanDesc)), n


VAR_COMMON = dict(abi=capi.RF_ABI, dtype=capi.RF_F32, n_planes=1, n_scans=None, device=HOST, flags=0, null=False)


def call_var_create(kind, f):
    L = capi.lib()
    d = {"image": capi.VarDesc, "signal": capi.VarSignalDesc, "volume": capi.VarVolumeDesc}[kind]()
    keep, pointer, n_scans = scan_array(f)
    d.abi, d.dtype, d.n_planes, d.n_weights, d.n_scans, d.device, d.flags = f["abi"], f["dtype"], f["n_planes"], f["n_weights"], n_scans, f["device"], f["flags"]
    if pointer is not None:
        d.scans = pointer
    if kind == "image":
        d.ndim = f["ndim"]
        d.extent[0], d.extent[1], d.extent[2] = f["width"], f["height"], f["depth"]
    elif kind == "signal":
        d.length = f["length"]
    else:
        d.width, d.height, d.depth = f["width"], f["height"], f["depth"]
    create = {"image": L.rf_var_plan_create, "signal": L.rf_var_plan_create_signal, "volume": L.rf_var_plan_create_volume}[kind]
    h = ctypes.c_void_p()
    status = create(None if f["null"] else ctypes.byref(d), ctypes.byref(h))
    del keep
    return answer(status, h, "rf_var_plan_destroy")


SMOOTH_COMMON = dict(abi=capi.RF_ABI, image_u8=0, width=64, height=40, n_planes=1, n_guide=0, guide_u8=0, iterations=2, sigma_s=40.0, sigma_r=0.5,
                     device=HOST, flags=0, null=False)


def call_smooth_create(kind, f):
    L = capi.lib()
    d = capi.SmoothVolumeDesc() if kind == "volume" else capi.SmoothDesc()
    for name in ("abi", "image_u8", "width", "height", "n_planes", "n_guide", "guide_u8", "iterations", "sigma_s", "sigma_r", "device", "flags"):
        setattr(d, name, f[name])
    h = ctypes.c_void_p()
    desc = None if f["null"] else ctypes.byref(d)
    if kind == "volume":
        d.depth, d.spacing_z = f["depth"], f["spacing_z"]
        status = L.rf_smooth_plan_create_volume(desc, ctypes.byref(h))
    elif kind == "batch":
        b = capi.SmoothBatchDesc()
        b.batch, b.image_stride, b.guide_stride = f["batch"], f["image_stride"], f["guide_stride"]
        status = L.rf_smooth_plan_create_batched(desc, None if f["null_batch"] else ctypes.byref(b), ctypes.byref(h))
    else:
        status = L.rf_smooth_plan_create(desc, ctypes.byref(h))
    return answer(status, h, "rf_smooth_plan_destroy")


def call_distances(kind, f):
    L = capi.lib()
    guide = arr(f["guide"])
    n_guide = f["n_guide"] if f["n_guide"] is not None else len(f["guide"])
    if kind == "image":
        status = L.rf_var_distances(guide, n_guide, f["guide_u8"], f["width"], f["height"], f["scale"], f["dx"], f["dy"], -1, None)
    elif kind == "volume":
        status = L.rf_var_distances_volume(guide, n_guide, f["guide_u8"], f["width"], f["height"], f["depth"], f["scale"], f["spacing_z"],
                                           f["dx"], f["dy"], f["dz"], -1, None)
    elif kind == "image_backward":
        status = L.rf_var_distances_backward(guide, n_guide, f["width"], f["height"], f["scale"], f["dx"], f["dy"], arr(f["grads"]), f["accumulate"], -1, None)
    else:
        status = L.rf_var_distances_volume_backward(guide, n_guide, f["width"], f["height"], f["depth"], f["scale"], f["dx"], f["dy"], f["dz"],
                                                    arr(f["grads"]), f["accumulate"], -1, None)
    return answer(status)


# ---- the tables: per entry point (name, call, baseline, faults in the validator's order, further cases) ------------------------
def scan_faults(dim_scans, weights_scans, both_scans):
    """abi .. the scan loop, alike in the three kinds but for rf_var_desc's ndim and the highest dim"""
    return [fault("abi", dict(abi=capi.RF_ABI + 1)),
            fault("flags", dict(flags=4)),
            fault("n_planes", dict(n_planes=capi.RF_MAX_PLANES + 1)),
            fault("n_weights", dict(n_weights=0)),
            fault("n_scans", dict(n_scans=capi.RF_VAR_MAX_SCANS + 1), dict(n_scans=0, scans=None)),
            fault("null_scans", dict(scans=None)),
            fault("dtype", dict(dtype=capi.RF_F64)),
            fault("scan_dim", dict(scans=dim_scans), dict(scans=both_scans)),
            fault("scan_weights", dict(scans=weights_scans))]


IMAGE_FAULTS = scan_faults([(0, 1, 0), (2, 0, 1)], [(0, 1, 0), (1, 0, 2)], [(0, 1, 0), (2, 0, 2)])
IMAGE_FAULTS.insert(6, fault("ndim", dict(ndim=3)))
IMAGE_FAULTS += [fault("extent_positive", dict(height=0)),
                 fault("extent_above", dict(width=MAXE + 4), dict(width=MAXE + 2)),
                 fault("width_multiple_of_4", dict(width=62))]

SIGNAL_FAULTS = scan_faults([(0, 1, 0), (1, 0, 0)], [(0, 1, 0), (0, 0, 1)], [(0, 1, 0), (1, 0, 1)])
SIGNAL_FAULTS += [fault("length_positive", dict(length=0), EXCLUSIVE),
                  fault("length_above", dict(length=(1 << 30) + 4), dict(length=(1 << 30) + 2)),
                  fault("length_multiple_of_4", dict(length=4098))]

VOLUME_DOMAIN = [fault("extents_above", dict(height=MAXE + 1)),
                 fault("width_multiple_of_4", dict(width=62), dict(width=(1 << 15) + 2, height=1 << 15)),
                 fault("width_times_height", dict(width=1 << 15, height=(1 << 15) + 4)),
                 fault("depth_on_grid_z", dict(depth=65536))]
VOLUME_FAULTS = scan_faults([(0, 1, 0), (3, 0, 1)], [(0, 1, 0), (1, 0, 3)], [(0, 1, 0), (3, 0, 3)])
VOLUME_FAULTS += [fault("extents_positive", dict(depth=0))] + VOLUME_DOMAIN

SMOOTH_FAULTS = [fault("abi", dict(abi=capi.RF_ABI + 1)),
                 fault("flags", dict(flags=1)),
                 fault("n_planes", dict(n_planes=0)),
                 fault("n_guide", dict(n_guide=-1)),
                 fault("image_u8", dict(image_u8=2)),
                 fault("guide_u8", dict(guide_u8=2), EXCLUSIVE),
                 fault("guide_u8_without_guide", dict(guide_u8=1)),
                 fault("iterations", dict(iterations=capi.RF_SMOOTH_MAX_ITERATIONS + 1)),
                 fault("extents_positive", dict(height=0)),
                 fault("sigma_s", dict(sigma_s=0.0)),
                 fault("sigma_r", dict(sigma_r=-1.0)),
                 fault("width_multiple_of_4", dict(width=62)),
                 fault("extents_above", dict(height=MAXE + 1))]
# behind the description: sigma_s / sigma_r that is no f32 (its bases then round to 1 as well), and a base that rounds to 0
SMOOTH_CONSTANTS = [fault("scale_not_f32", dict(sigma_s=1e300, sigma_r=1e-300), dict(sigma_s=1e300, sigma_r=1e-300)),
                    fault("base_rounds", dict(sigma_s=1e-3))]

BATCH_FAULTS = [fault("null_batch", dict(null_batch=True)),
                fault("batch", dict(batch=0)),
                fault("strides_multiple_of_4", dict(image_stride=2562), dict(image_stride=2558)),
                fault("image_stride_below", dict(image_stride=2556)),
                fault("guide_stride_self_guided", dict(guide_stride=4), EXCLUSIVE),
                fault("guide_stride_below", dict(n_guide=1, guide_stride=2556))]

SMOOTH_VOLUME_FAULTS = ([SMOOTH_FAULTS[0], fault("flags", dict(flags=2))] + SMOOTH_FAULTS[2:] +
                        [fault("backward_of_bytes", dict(flags=1, image_u8=1)),
                         fault("spacing_z", dict(spacing_z=0.0)),
                         fault("depth_positive", dict(depth=0), EXCLUSIVE),
                         fault("depth_above", dict(depth=MAXE + 1))] + VOLUME_DOMAIN[2:] + SMOOTH_CONSTANTS)

DISTANCE_COMMON = dict(guide=[A], n_guide=None, guide_u8=0, width=64, height=40, scale=1.0, dx=B, dy=C)      # 64 x 40 f32: 0x2800 bytes
DISTANCE_HEAD = [fault("n_guide", dict(n_guide=0)),
                 fault("extents_positive", dict(height=0))]
DISTANCE_FAULTS = DISTANCE_HEAD + [
    fault("null_argument", dict(dx=None)),
    fault("null_guide_plane", dict(guide=[A, None])),
    fault("scale", dict(scale=-1.0)),
    fault("width_multiple_of_4", dict(width=62)),
    fault("extents_above", dict(height=MAXE + 1)),
    fault("outputs_aligned", dict(dy=C + 4)),
    fault("guide_aligned", dict(guide=[A + 4])),
    fault("outputs_overlap", dict(dy=B + 0x100)),
    fault("guide_overlaps_output", dict(guide=[B]))]
DISTANCE_VOLUME_FAULTS = DISTANCE_HEAD + [                                                                    # 64 x 40 x 8 f32: 0x14000 bytes
    fault("null_argument", dict(dz=None)),
    fault("null_guide_volume", dict(guide=[A, None])),
    fault("scale", dict(scale=-2.5)),
    fault("spacing_z", dict(spacing_z=0.0))] + VOLUME_DOMAIN + [
    fault("outputs_aligned", dict(dz=D + 4)),
    fault("guide_aligned", dict(guide=[A + 8])),
    fault("outputs_overlap", dict(dz=C + 0x100)),
    fault("guide_overlaps_output", dict(guide=[D]))]
BACKWARD_TAIL = [fault("gradients_aligned", dict(dy=C + 4)),
                 fault("guide_aligned", dict(guide=[A + 4])),
                 fault("gradient_overlaps_distance_gradient", dict(grads=[B + 0x100]), dict(dx=A, grads=[A])),
                 fault("gradient_overlaps_guide", dict(grads=[A]), dict(guide=[A, G], grads=[A + 0x100, A + 0x200])),
                 fault("gradient_overlaps_gradient", dict(guide=[A, G], grads=[E, E + 0x100]))]
BACKWARD_HEAD = DISTANCE_HEAD + [fault("null_argument", dict(dx=None)),
                                 fault("null_guide_or_gradient", dict(guide=[A, G], grads=[E, None])),
                                 fault("scale", dict(scale=float("inf")))]
DISTANCE_BACKWARD_FAULTS = BACKWARD_HEAD + [fault("accumulate", dict(accumulate=2)),
                                            fault("width_multiple_of_4", dict(width=62)),
                                            fault("extents_above", dict(height=MAXE + 1))] + BACKWARD_TAIL
DISTANCE_VOLUME_BACKWARD_FAULTS = BACKWARD_HEAD + VOLUME_DOMAIN + [fault("accumulate", dict(accumulate=2))] + BACKWARD_TAIL

ENTRY_POINTS = [
    ("rf_var_plan_create", lambda f: call_var_create("image", f),
     dict(VAR_COMMON, ndim=2, width=64, height=40, depth=0, n_weights=2, scans=[(0, 1, 0), (1, 0, 1)]), IMAGE_FAULTS,
     [("null_description", dict(null=True)),
      ("scan_0_weights+scan_1_dim", dict(scans=[(0, 1, 5), (2, 0, 1)])),
      ("extent_positive_both", dict(width=0, height=0))]),
    ("rf_var_plan_create_signal", lambda f: call_var_create("signal", f),
     dict(VAR_COMMON, length=4096, n_weights=1, scans=[(0, 1, 0), (0, 0, 0)]), SIGNAL_FAULTS,
     [("null_description", dict(null=True)),
      ("scan_0_weights+scan_1_dim", dict(scans=[(0, 1, 5), (1, 0, 0)])),
      ("length_positive+length_multiple_of_4", dict(length=-2))]),
    ("rf_var_plan_create_volume", lambda f: call_var_create("volume", f),
     dict(VAR_COMMON, width=64, height=40, depth=8, n_weights=3, scans=[(0, 1, 0), (1, 0, 1), (2, 1, 2)]), VOLUME_FAULTS,
     [("null_description", dict(null=True)),
      ("scan_0_weights+scan_1_dim", dict(scans=[(0, 1, 5), (3, 0, 1)])),
      ("depth_on_grid_z_by_planes", dict(depth=4096, n_planes=16))]),
    ("rf_smooth_plan_create", lambda f: call_smooth_create("image", f), SMOOTH_COMMON, SMOOTH_FAULTS + SMOOTH_CONSTANTS,
     [("null_description", dict(null=True))]),
    ("rf_smooth_plan_create_batched", lambda f: call_smooth_create("batch", f),
     dict(SMOOTH_COMMON, batch=2, image_stride=2560, guide_stride=0, null_batch=False), BATCH_FAULTS + SMOOTH_FAULTS + SMOOTH_CONSTANTS,
     [("null_description", dict(null=True))]),
    ("rf_smooth_plan_create_volume", lambda f: call_smooth_create("volume", f), dict(SMOOTH_COMMON, depth=8, spacing_z=1.0), SMOOTH_VOLUME_FAULTS,
     [("null_description", dict(null=True)),
      ("flags_other_bits_with_the_flag", dict(flags=3)),
      ("spacing_z_beyond_f32", dict(spacing_z=1e300))]),
    ("rf_var_distances", lambda f: call_distances("image", f), DISTANCE_COMMON, DISTANCE_FAULTS,
     [("byte_guide_aligned", dict(guide_u8=1, guide=[A + 2])),
      ("n_guide_above", dict(n_guide=capi.RF_MAX_PLANES + 1, guide=None))]),
    ("rf_var_distances_volume", lambda f: call_distances("volume", f), dict(DISTANCE_COMMON, depth=8, spacing_z=1.0, dz=D), DISTANCE_VOLUME_FAULTS,
     [("byte_guide_aligned", dict(guide_u8=1, guide=[A + 2])),
      ("spacing_z+width_multiple_of_4", dict(spacing_z=-1.0, width=62)),
      ("dx_overlaps_dy", dict(dy=B + 0x100))]),
    ("rf_var_distances_backward", lambda f: call_distances("image_backward", f), dict(DISTANCE_COMMON, grads=[E], accumulate=0), DISTANCE_BACKWARD_FAULTS,
     [("accumulate+extents_above", dict(accumulate=-1, height=MAXE + 1)),
      ("gradient_overlaps_dy", dict(grads=[C]))]),
    ("rf_var_distances_volume_backward", lambda f: call_distances("volume_backward", f), dict(DISTANCE_COMMON, depth=8, dz=D, grads=[E], accumulate=0),
     DISTANCE_VOLUME_BACKWARD_FAULTS,
     [("width_multiple_of_4+accumulate", dict(width=62, accumulate=2)),
      ("gradient_overlaps_dz", dict(grads=[D + 0x13ff0]))]),
]


def cases():
    """[(case id, call, arguments)]: per entry point every fault alone, every consecutive pair, then the further cases"""
    out = []
    for entry, call, baseline, faults, further in ENTRY_POINTS:
        for i, (name, single, with_next) in enumerate(faults):
            out.append((f"{entry}:{name}", call, dict(baseline, **single)))
            if i + 1 < len(faults) and with_next != EXCLUSIVE:
                both = with_next if with_next is not None else dict(single, **faults[i + 1][1])
                assert with_next is not None or not set(single) & set(faults[i + 1][1]), f"{entry}:{name}: the pair needs overrides of its own"
                out.append((f"{entry}:{name}+{faults[i + 1][0]}", call, dict(baseline, **both)))
        out += [(f"{entry}:{name}", call, dict(baseline, **overrides)) for name, overrides in further]
    assert len({case_id for case_id, _, _ in out}) == len(out)
    return out


CASES = cases()


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as fh:
        return {case_id: (status, text) for case_id, status, text in json.load(fh)}


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(recorded()) == sorted(case_id for case_id, _, _ in CASES)


def test_every_entry_point_is_covered():
    assert [e[0] for e in ENTRY_POINTS] == ["rf_var_plan_create", "rf_var_plan_create_signal", "rf_var_plan_create_volume", "rf_smooth_plan_create",
                                            "rf_smooth_plan_create_batched", "rf_smooth_plan_create_volume", "rf_var_distances",
                                            "rf_var_distances_volume", "rf_var_distances_backward", "rf_var_distances_volume_backward"]
    ids = {case_id for case_id, _, _ in CASES}
    # the precedences that differ between the two backwards, and spacing_z against the volume domain
    assert {"rf_var_distances_backward:accumulate+width_multiple_of_4", "rf_var_distances_backward:accumulate+extents_above",
            "rf_var_distances_volume_backward:width_multiple_of_4+accumulate", "rf_var_distances_volume_backward:depth_on_grid_z+accumulate",
            "rf_var_distances_volume:spacing_z+extents_above", "rf_var_distances_volume:spacing_z+width_multiple_of_4",
            "rf_smooth_plan_create_volume:spacing_z+depth_positive"} <= ids


@pytest.mark.parametrize("case_id,call,arguments", CASES, ids=[c[0] for c in CASES])
def test_refusal(case_id, call, arguments):
    want_status, want_text = recorded()[case_id]
    status, text = call(arguments)
    assert status != capi.RF_OK, "every case is a refusal"
    assert (status, text) == (want_status, want_text)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_var_refusals_host.py --record   (on a build from before the change the fixture is to check)")
    rows = []
    for case_id, call, arguments in CASES:
        status, text = call(arguments)
        assert status != capi.RF_OK, f"{case_id}: accepted"
        rows.append([case_id, status, text])
    with open(FIXTURE, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} cases -> {FIXTURE}")
