# Round-3 session run for the judged artifacts: every GPU test, smoke, the
# bench line, rocprof kernel stats + FETCH/WRITE PMC passes of the bench
# kernels, the FFV1 line with its kernel stats, config 3/4 lines.
# Usage (through gpurun): bash tools/gpu_final_r3.sh TAG
set -o pipefail
TAG=${1:-r3f}
mkdir -p ${OUT:-bench_out}
export TMPDIR=/tmp
timeout -k 10 800 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread > ${OUT:-bench_out}/pytest_gpu_$TAG.log 2>&1; rc=$?
echo "pytest rc=$rc"; tail -2 ${OUT:-bench_out}/pytest_gpu_$TAG.log; grep -E "^(FAILED|ERROR)" ${OUT:-bench_out}/pytest_gpu_$TAG.log | head -20
if [ $rc -gt 1 ]; then echo "stopping after pytest rc=$rc"; exit $rc; fi
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > ${OUT:-bench_out}/smoke_$TAG.log 2>&1 || { tail -5 ${OUT:-bench_out}/smoke_$TAG.log; exit 1; }
tail -1 ${OUT:-bench_out}/smoke_$TAG.log
timeout -k 10 400 python -u bench.py --full > ${OUT:-bench_out}/bench_$TAG.json 2> ${OUT:-bench_out}/bench_$TAG.err || { tail -5 ${OUT:-bench_out}/bench_$TAG.err; exit 1; }
python3 -c "import json;d=json.load(open('${OUT:-bench_out}/bench_$TAG.json'));print('value',d['value'],'frac',d['roofline']['frac'],'ms',d['roofline']['avg_launch_ms'],'siti',d['siti_kernel']['avg_launch_ms'],'pcie',d.get('pcie_pipeline',{}).get('frames_per_s'),'cpu',d['cpu_baseline']['value'],'e2e',d['e2e_avpvs']['frames_per_s'])"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d ${OUT:-bench_out}/prof_kt_$TAG -o run -- python3 bench.py --full --steps 10 --warmup 2 --pvs-total 4 --pool 4 --no-cpu-baseline --no-pipeline --no-siti-file --no-e2e > ${OUT:-bench_out}/prof_kt_$TAG.log 2>&1 || { tail -5 ${OUT:-bench_out}/prof_kt_$TAG.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d ${OUT:-bench_out}/prof_fetch_$TAG -o run -- python3 bench.py --full --steps 2 --warmup 0 --pvs-total 2 --pool 2 --no-cpu-baseline --no-pipeline --no-siti-file --no-e2e > ${OUT:-bench_out}/prof_fetch_$TAG.log 2>&1 || { tail -5 ${OUT:-bench_out}/prof_fetch_$TAG.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d ${OUT:-bench_out}/prof_write_$TAG -o run -- python3 bench.py --full --steps 2 --warmup 0 --pvs-total 2 --pool 2 --no-cpu-baseline --no-pipeline --no-siti-file --no-e2e > ${OUT:-bench_out}/prof_write_$TAG.log 2>&1 || { tail -5 ${OUT:-bench_out}/prof_write_$TAG.log; exit 1; }
python3 tools/pmc_traffic.py ${OUT:-bench_out}/prof_fetch_$TAG/run_counter_collection.csv ${OUT:-bench_out}/prof_write_$TAG/run_counter_collection.csv ${OUT:-bench_out}/prof_kt_$TAG/run_kernel_trace.csv ${OUT:-bench_out}/pmc_traffic_$TAG.json 600 > /dev/null || exit 1
grep -E "pp::" ${OUT:-bench_out}/prof_kt_$TAG/run_kernel_stats.csv | cut -d, -f1-4 | cut -c1-140
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d ${OUT:-bench_out}/kt_ffv1_$TAG -o run -- python3 bench.py --full --workload ffv1 --ffv1-concurrent 1 --steps 2 --warmup 1 > ${OUT:-bench_out}/bench_ffv1_$TAG.json 2> ${OUT:-bench_out}/bench_ffv1_$TAG.err || { tail -5 ${OUT:-bench_out}/bench_ffv1_$TAG.err; exit 1; }
grep -E "ffv1" ${OUT:-bench_out}/kt_ffv1_$TAG/run_kernel_stats.csv | cut -d, -f1-4
for wl in config3-10 config3-8 config4; do
  timeout -k 10 200 python -u bench.py --full --workload $wl --steps 10 --warmup 2 --no-cpu-baseline --no-pipeline > ${OUT:-bench_out}/bench_${wl}_$TAG.json 2>> ${OUT:-bench_out}/bench_$TAG.err || { tail -3 ${OUT:-bench_out}/bench_$TAG.err; exit 1; }
  cut -c1-200 ${OUT:-bench_out}/bench_${wl}_$TAG.json
done
