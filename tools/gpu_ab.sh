#!/bin/bash
# A/B timing of library variants on the GPU box: tools/gpu_ab.sh <output dir> <tag> [ENV=VAL,...]...   each argument = one run of the NS bench at 400 loci
OUT=$1; TAG=$2; shift 2
mkdir -p $OUT
O=$OUT/ab_$TAG.txt
for v in "$@"; do
  envs=$(echo "$v" | tr ',' ' ')
  echo "== $v" >> $O
  env $envs python bench.py --full --loci ${AB_LOCI:-400} --steps 3 --warmup 1 --no-cpu-baseline --no-pipeline 2>$OUT/ab_${TAG}_err.txt | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(round(d['value']/1e6,2), 'M/s pass_ms', round(d['roofline']['pass_ms'],2), {k:round(v,2) for k,v in d['roofline']['phase_ms'].items()})" >> $O 2>&1
done
cat $O
