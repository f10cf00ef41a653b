#!/bin/bash
# Register, LDS and scratch figures of every kernel in some .hip files of two source trees (hipcc's kernel-resource-usage
# remarks, device code only), one line per kernel: "same" or old -> new.
#   bash tools/kernel_resources.sh OLD_TREE NEW_TREE kernels_tails.hip kernels_tails_mfma.hip kernels_fused_tall.hip
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
old=$1; new=$2; shift 2
tmp=$(mktemp -d)
for f in "$@"; do
  for side in old new; do
    tree=$old; [ $side = new ] && tree=$new
    $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize --cuda-device-only -Rpass-analysis=kernel-resource-usage \
      -c $tree/recfilter_amd/csrc/$f -o /dev/null 2> $tmp/$side.$f.txt &
  done
done
wait
python3 - "$tmp" "$@" <<'EOF'
import re, subprocess, sys
tmp, files = sys.argv[1], sys.argv[2:]
filt = "c++filt"      # (leaves names with _Float16 / __bf16 arguments mangled: matched as they are)
def parse(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: .*?(Function Name|VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            name = subprocess.run([filt, v], capture_output=True, text=True).stdout.strip()
            out[name] = {}
        elif name:
            out[name][k.split(" ")[0]] = v
    return out
fmt = lambda d: "vgpr %s agpr %s sgpr %s scratch %s lds(static) %s waves/SIMD %s" % tuple(d.get(k, "?") for k in ("VGPRs", "AGPRs", "SGPRs", "ScratchSize", "LDS", "Occupancy"))
for f in files:
    o, n = parse(f"{tmp}/old.{f}.txt"), parse(f"{tmp}/new.{f}.txt")
    print(f"== {f}: {len(o)} kernels before, {len(n)} after")
    # a template parameter added at the end of a kernel's list shows in the names of the new tree: match on the old name's arguments
    # (a trailing type parameter with a default shows as ", float>(")
    key = lambda name: re.sub(r", (false|float)>\(", ">(", name).replace("Lb0EEEv", "EEv", 1)
    nk = {}
    for name in n:
        nk.setdefault(key(name), name)
    same = 0
    for name, d in sorted(o.items()):
        m = n.get(name) or n.get(nk.get(name, ""))
        if m is None:
            print(f"  GONE {name}")
        elif m == d:
            same += 1
        else:
            print(f"  CHANGED {name}\n     old: {fmt(d)}\n     new: {fmt(m)}")
    print(f"  {same} of {len(o)} existing kernels: same")
    matched = set(o) | {nk[k] for k in nk if k in o}
    for name, d in sorted(n.items()):
        if name not in matched:
            print(f"  NEW {name}\n     {fmt(d)}")
EOF
