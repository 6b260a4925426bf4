# Zero-copy (kernel reads pinned host memory over PCIe) vs segmented H2D, for batch shapes of the
# uploads dispatcher:  bash tools/gpu_zero_copy.sh "<chunks> <chunk_bytes>" ...
cd "$(dirname "$0")/.." || exit 1; mkdir -p ${OUT_DIR:-out}/zc
for spec in "$@"; do
  set -- $spec
  timeout -k 10 300 python bench.py --full --chunks $1 --chunk-bytes $2 --host-inclusive on --no-cpu-baseline --ingest-leg off --mixed-leg off --steps 3 --warmup 1 > ${OUT_DIR:-out}/zc/c$1_b$2.json 2> ${OUT_DIR:-out}/zc/err || { echo "FAIL $spec"; tail -5 ${OUT_DIR:-out}/zc/err; exit 1; }
  python3 -c "import json;d=json.load(open('${OUT_DIR:-out}/zc/c$1_b$2.json'));h=d['host_inclusive'];print('$1 x $2', 'device', d['value'], 'segmented', h['value'], 'zero-copy', h['zero_copy_value'], d['config'].get('kernel'))"
done
