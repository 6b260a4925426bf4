cd "$(dirname "$0")/.." || exit 1; mkdir -p ${OUT_DIR:-out}
timeout -k 10 1100 python bench.py --full --workload ingest --ingest-batch 131072 --warmup 0 --progress > ${OUT_DIR:-out}/cfg_ingest.json 2> ${OUT_DIR:-out}/cfg_ingest.err; rc=$?
echo "ingest rc=$rc"; cat ${OUT_DIR:-out}/cfg_ingest.json; grep -v amdgpu ${OUT_DIR:-out}/cfg_ingest.err | tail -5; exit $rc
