# host-to-host bench A/B of two library builds (no profiled replay, no CPU baseline), 2 reps each
# lines go to $OF_OUT/bench_ab.log (default out/)
set -e
O=${OF_OUT:-out}
mkdir -p $O
: > $O/bench_ab.log
for rep in 1 2; do for L in "$@"; do
  echo "== $L rep $rep" >> $O/bench_ab.log
  OPTFLOW_LIB=$L timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-profile 2>/dev/null | grep '^{' >> $O/bench_ab.log
done; done
