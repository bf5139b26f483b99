# rocprofv3 kernel trace of the default bench (sub-cycle + full RK3 steps); summary written by scripts/summarize_db.py
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT_ROOT:-results}/final_prof
rm -rf $OUT; mkdir -p $(dirname $OUT)
rocprofv3 --kernel-trace --stats -d $OUT -o final -- python3 bench.py --full --no-cpu-baseline --steps 5 --warmup 2 > $OUT.log 2>&1
tail -1 $OUT.log | cut -c1-300
python3 scripts/summarize_db.py $OUT/final_results.db
