#!/bin/bash
# k_remap_u8 alone (scripts/undistort_image_rate.py --kernel-only: nothing but uploads of a rectified 4-camera 720p rig), for 128 and
# 512 images per launch: its time from a rocprofv3 --kernel-trace --stats run, and fetched / written bytes from counter runs of their
# own (no tracing in the same run).  Run on the GPU box from the repo root:
#   bash scripts/undistort_image_profile.sh <outdir>
O=${1:-profiles_out/udi}
mkdir -p $O
ROOT=$(pwd)
cd /tmp && export TMPDIR=/tmp && cd $ROOT
step() { "$@" || { echo "step failed ($?): $*"; exit 1; }; }
for n in 128 512; do
    step timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/st$n -o s -- python3 scripts/undistort_image_rate.py --kernel-only $n > $O/st$n.log 2>&1
    f=$(find $O/st$n -name '*kernel_stats.csv' | head -1); [ -n "$f" ] && cp $f $O/remap_${n}_kernel_stats.csv && grep -i "name\|k_remap" $O/remap_${n}_kernel_stats.csv | cut -d, -f1-8
    for c in FETCH_SIZE WRITE_SIZE; do
        step timeout -k 10 240 rocprofv3 --pmc $c --output-format csv -d $O/pm${n}_$c -o p -- python3 scripts/undistort_image_rate.py --kernel-only $n > $O/pm${n}_$c.log 2>&1
        f=$(find $O/pm${n}_$c -name '*counter_collection.csv' | head -1)
        [ -n "$f" ] && python3 scripts/pmc_summary.py $f > $O/remap_${n}_$c.txt && grep -A4 "^k_remap" $O/remap_${n}_$c.txt
    done
    rm -rf $O/st$n $O/pm${n}_FETCH_SIZE $O/pm${n}_WRITE_SIZE
done
