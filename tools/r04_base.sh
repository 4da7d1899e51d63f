set -x
out=${1:?usage: tools/r04_base.sh <output directory>}; mkdir -p $out
for wl in p30 c2 ns; do
  HIPSTR_HOST_THREADS=2 timeout 600 python bench.py --full --workload $wl --no-cpu-baseline --steps 5 > $out/${wl}_t2.json 2> $out/${wl}_t2.err
  timeout 600 python bench.py --full --workload $wl --no-cpu-baseline --steps 5 > $out/${wl}_t16.json 2> $out/${wl}_t16.err
done
nproc; cat /sys/fs/cgroup/cpu.max; lscpu | head -20
