#!/bin/bash
# rocprofv3 evidence for every kernel other than the timed one: tools/bench_aux.py under --kernel-trace --stats and
# under separate --pmc FETCH_SIZE / WRITE_SIZE passes.   bash tools/run_profiles_aux.sh r02   (GPU box, repo root)
# -> gpurun_out/<tag>_aux.jsonl (the program's own HIP-event timings), prof_aux_stats/, prof_aux_fetch/, prof_aux_write/
# Every step runs under its own time limit; the first step that fails ends the recipe with its exit status.
set -u
TAG=${1:-r02}
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
O=$R/gpurun_out
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
export REPS=${REPS:-5}

# step <seconds> <log> <command...>: run one step, stop the recipe if it fails
step() {
	local t=$1 log=$2
	shift 2
	timeout -k 10 $t "$@" > $log 2>&1
	local rc=$?
	if [ $rc -ne 0 ]; then
		echo "run_profiles_aux.sh: step failed with exit status $rc (log: $log): $*" >&2
		tail -20 $log >&2
		exit $rc
	fi
}

step 900 $O/${TAG}_aux.err rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_aux_stats -o ${TAG}_aux -- python3 $R/tools/bench_aux.py
grep '^{"kernel"' $O/${TAG}_aux.err > $O/${TAG}_aux.jsonl
export REPS=1
for C in FETCH_SIZE WRITE_SIZE; do
	d=$O/prof_aux_$(echo $C | tr A-Z a-z | sed 's/_size//')
	step 900 $O/${TAG}_aux_$C.log rocprofv3 --output-format csv --pmc $C -d $d -o ${TAG}_aux -- python3 $R/tools/bench_aux.py
done
find $O/prof_aux_stats $O/prof_aux_fetch $O/prof_aux_write -name "*kernel_trace.csv" -delete
find $O/prof_aux_stats $O/prof_aux_fetch $O/prof_aux_write -name "*agent_info.csv" -delete
# counter files: keep the library's kernels only (drop torch's fill / copy / rng kernels)
for f in $(find $O/prof_aux_fetch $O/prof_aux_write -name "*counter_collection.csv"); do
	(head -1 $f; grep -E "burst_pull|pack_trxd|va_demod|channelize|resample|frontend_fused|convolve_kernel|convolve_lds_kernel|convert_short|delay_vector|energy_detect|vector_slicer|sch_detect|save_" $f) > $f.tmp && mv $f.tmp $f
done
du -sh $O/prof_aux_*
cat $O/${TAG}_aux.jsonl
