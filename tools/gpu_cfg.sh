# Full-size BASELINE configs beyond the default: concurrent uploads, mixed (configs[3]).
cd "$(dirname "$0")/.." || exit 1; mkdir -p ${OUT_DIR:-out}
timeout -k 10 300 python bench.py --workload uploads > ${OUT_DIR:-out}/cfg_uploads.json 2> ${OUT_DIR:-out}/cfg_uploads.err; rc=$?
echo "uploads rc=$rc"; cat ${OUT_DIR:-out}/cfg_uploads.json; [ $rc -eq 0 ] || { tail -5 ${OUT_DIR:-out}/cfg_uploads.err; exit $rc; }
timeout -k 10 600 python bench.py --full --workload mixed --mixed-chunks 65536 --warmup 0 --progress > ${OUT_DIR:-out}/cfg_mixed.json 2> ${OUT_DIR:-out}/cfg_mixed.err; rc=$?
echo "mixed rc=$rc"; cat ${OUT_DIR:-out}/cfg_mixed.json; tail -3 ${OUT_DIR:-out}/cfg_mixed.err; exit $rc
