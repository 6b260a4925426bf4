# A/B builds of the library on the SAME device, interleaved 3x:
#   LIBS="libefeshash_va.so libefeshash_vb.so" bash tools/gpu_ab.sh [bench args]
cd "$(dirname "$0")/.." || exit 1; mkdir -p ${OUT_DIR:-out}
for rep in 1 2 3; do
  for lib in $LIBS; do
    EFES_LIB_OVERRIDE=$PWD/efes_amd/lib/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --host-inclusive off --ingest-leg off --mixed-leg off "$@" > ${OUT_DIR:-out}/ab.json 2> ${OUT_DIR:-out}/ab.err || { echo "FAIL $lib"; tail -5 ${OUT_DIR:-out}/ab.err; exit 1; }
    python -c "import json,sys;d=json.load(open('${OUT_DIR:-out}/ab.json'));print(sys.argv[1], d['value'], 'GiB/s', d['roofline']['kernel_ms'],'ms/launch')" $lib
  done
done
