# What the driver does at round end, on one GPU box: the GPU suite with -x, smoke(), the default bench line with 5 + 20 steps
# (plain, as it is timed, and once with --full).
#   bash tools/driver_rehearsal.sh <outdir>
out=${1:?usage: bash tools/driver_rehearsal.sh <outdir>}
mkdir -p $out
python -m pytest tests -x -q -m gpu > $out/suite_run_x.log 2>&1; echo "suite (-x, as the driver runs it) rc=$?"; tail -2 $out/suite_run_x.log
python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.log 2>&1; echo smoke rc=$?; tail -1 $out/smoke.log
python bench.py --steps 20 --warmup 5 > $out/bench_driver_protocol.json 2> $out/bench_driver_protocol.err; echo bench rc=$?
python bench.py --steps 20 --warmup 5 --full > $out/bench_full.json 2> $out/bench_full.err; echo bench --full rc=$?
python -c "
import json, sys
d, f = (json.load(open(p)) for p in sys.argv[1:3])
print(d['ms_per_step'], f['ms_per_step_steady'], f['roofline']['frac'], f['roofline']['traffic'], f['configs'][0]['ms_per_step'], f['configs'][0]['roofline']['traffic'])
" $out/bench_driver_protocol.json $out/bench_full.json
