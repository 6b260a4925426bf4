cd "$(dirname "$0")/.." || exit 1; mkdir -p ${OUT_DIR:-out}
run() {  # run one bench configuration, print a summary line; stop the sweep on any failure
  timeout -k 10 ${T:-300} python bench.py --full --no-cpu-baseline --host-inclusive off --ingest-leg off --mixed-leg off "$@" > ${OUT_DIR:-out}/b.json 2> ${OUT_DIR:-out}/b.err || { echo "FAIL $*"; tail -5 ${OUT_DIR:-out}/b.err; exit 1; }
  python -c "import json,sys;d=json.load(open('${OUT_DIR:-out}/b.json'));print(sys.argv[1:], d['value'], 'GiB/s', d['roofline']['kernel_ms'],'ms/launch', d['steps'], 'steps', d['config']['kernel'], d['config'].get('bytes_per_gpu',''))" "$@"
  cp ${OUT_DIR:-out}/b.json "${OUT_DIR:-out}/sweep_$(echo "$*" | tr ' -' '__').json"
}
for spec in "$@"; do eval run $spec; done
echo SWEEP_DONE
