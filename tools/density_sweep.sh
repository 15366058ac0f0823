# join grid density sweep on one box (bench join leg: the join and the row predicate), densities from
# $DENS (default "16384 20480"), two alternating rounds; records go to $DOUT (default bench_out/)
i=0
odir=${DOUT:-bench_out}
mkdir -p "$odir"
for r in 1 2; do
  for c in ${DENS:-16384 20480}; do
    i=$((i+1))
    o=$odir/${DTAG:-dens}_${c}_$i
    timeout -k 10 300 python -u bench.py --full --only join --no-cpu --no-gather --steps 1 --warmup 0 --join-steps 3 --cells-per-poly $c > $o.json 2> $o.err || exit 1
    grep '^BENCH_DETAIL ' $o.err | tail -n 1 | cut -c 14- > $o.detail.json
  done
done
