# A/B of library builds over several bench workloads (same device, interleaved):
#   LIBS="a.so b.so" REPS=2 bash tools/gpu_ab_multi.sh "<bench args 1>" "<bench args 2>" ...
cd "$(dirname "$0")/.." || exit 1; mkdir -p ${OUT_DIR:-out}
for rep in $(seq 1 ${REPS:-2}); do
  for args in "$@"; do
    for lib in $LIBS; do
      EFES_LIB_OVERRIDE=$PWD/efes_amd/lib/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --host-inclusive off --ingest-leg off --mixed-leg off $args > ${OUT_DIR:-out}/abm.json 2> ${OUT_DIR:-out}/abm.err || { echo "FAIL $lib $args"; tail -5 ${OUT_DIR:-out}/abm.err; exit 1; }
      python -c "import json,sys;d=json.load(open('${OUT_DIR:-out}/abm.json'));print(sys.argv[1], '|', sys.argv[2], '|', d['value'], 'GiB/s', d['roofline']['kernel_ms'],'ms')" $lib "$args"
    done
  done
done
