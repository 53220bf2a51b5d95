# kernel + memory-copy timeline of the e2e_avpvs leg (no PMC counters).
set -o pipefail
mkdir -p ${OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
rm -rf ${OUT:-bench_out}/e2etrace
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d ${OUT:-bench_out}/e2etrace -- python3 -u bench.py --full --steps 1 --warmup 0 --pvs-total 4 --no-cpu-baseline --no-pipeline --no-siti-file > ${OUT:-bench_out}/e2etrace.json 2> ${OUT:-bench_out}/e2etrace.err || { tail -20 ${OUT:-bench_out}/e2etrace.err; exit 1; }
python3 tools/e2e_trace.py ${OUT:-bench_out}/e2etrace 1.6 > ${OUT:-bench_out}/e2etrace_summary.txt
python3 -c "import json;d=json.load(open('${OUT:-bench_out}/e2etrace.json'));e=d['e2e_avpvs'];print(e['frames_per_s'], e['single_pvs']['frames_per_s']);print(json.dumps(e['stages']))"
head -c 3000 ${OUT:-bench_out}/e2etrace_summary.txt
