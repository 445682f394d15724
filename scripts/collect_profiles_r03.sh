#!/bin/bash
# Round-3 judged profiles (run through gpurun from the repo root): scripts/collect_profiles_r03.sh <tag>
#  1. rocprofv3 --kernel-trace --stats of the default bench command and of --timed-only (+ split by grid size)
#  2. the same for --cells 1024 (working sets >> 256 MiB Infinity Cache)
#  3. separate --pmc FETCH_SIZE / WRITE_SIZE passes of the default workload, tgv3d n=64 and channel3d n=64
#  4. traces of the 3D workloads
#  5. plain bench lines (no profiler) of every workload; smoother launch cold / warm sweeps; the one-step kernels
#     (NSFEM_LATTICE=0) for comparison; ordering experiments (DFG: lex / morton / rcm; 3D: lex / parity)
TAG=${1:-r03_x}
REPO=$(pwd); O=$REPO/gpurun_out/$TAG
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
trace() {  # name, bench args...
  local name=$1; shift
  timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/t_$name -o b -- python3 $REPO/bench.py "$@" > $O/${TAG}_$name.json 2> $O/t_$name.err
  cp $(find $O/t_$name -name "*kernel_stats.csv" | head -1) $O/${TAG}_${name}_kernel_stats.csv
  python3 $REPO/scripts/summarize_trace_by_grid.py $(find $O/t_$name -name "*kernel_trace.csv" | head -1) 500 > $O/${TAG}_${name}_kernel_stats_by_grid.csv
  rm -rf $O/t_$name
  echo "trace $name done: $(tail -c 300 $O/${TAG}_$name.json | head -c 120)"
}
pmc() {  # name, bench args...
  local name=$1; shift
  for C in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 500 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $O/p_${name}_$C -o b -- python3 $REPO/bench.py "$@" > /dev/null 2> $O/p_${name}_$C.err
  done
  python3 $REPO/scripts/summarize_pmc.py $O/p_${name}_FETCH_SIZE $O/p_${name}_WRITE_SIZE > $O/${TAG}_${name}_pmc_fetch_write_size.json
  rm -rf $O/p_${name}_FETCH_SIZE $O/p_${name}_WRITE_SIZE
  echo "pmc $name done"
}
trace bench_n512 --full --steps 20 --warmup 5 --no-cpu-baseline
trace bench_n512_timed_steps_only --steps 40 --warmup 10 --timed-only
trace bench_n1024 --full --cells 1024 --steps 5 --warmup 2 --no-cpu-baseline --no-solver-classes
trace tgv3d_n64 --workload tgv3d-ipcs --cells 64 --steps 5 --warmup 2
trace channel3d_n48 --workload channel3d-bdf --cells 48 --steps 3 --warmup 2
export NSFEM_LATTICE=0
trace bench_n512_one_step_kernels --steps 40 --warmup 10 --timed-only
unset NSFEM_LATTICE
pmc bench_n512 --steps 1 --warmup 1 --timed-only
pmc bench_n1024 --cells 1024 --steps 1 --warmup 1 --timed-only
pmc tgv3d_n64 --workload tgv3d-ipcs --cells 64 --steps 1 --warmup 1
pmc channel3d_n64 --workload channel3d-bdf --cells 64 --steps 1 --warmup 1
cd $REPO
timeout -k 10 900 python3 bench.py --full > $O/${TAG}_bench_default.json 2> $O/bench_default.err
timeout -k 10 600 python3 bench.py --full --cells 1024 --steps 20 --warmup 3 --no-cpu-baseline --no-solver-classes > $O/${TAG}_bench_n1024.json 2> $O/bench_1024.err
timeout -k 10 600 python3 bench.py --full --cells 333 --steps 50 --warmup 5 --no-cpu-baseline > $O/${TAG}_bench_n333.json 2> $O/bench_333.err
timeout -k 10 600 python3 bench.py --workload channel3d-bdf --cells 64 --steps 10 --warmup 3 > $O/${TAG}_bench_channel3d_n64.json 2> $O/bench_ch64.err
timeout -k 10 600 python3 bench.py --workload channel3d-bdf --cells 48 --steps 10 --warmup 3 > $O/${TAG}_bench_channel3d_n48.json 2> $O/bench_ch48.err
timeout -k 10 600 python3 bench.py --workload tgv3d-ipcs --cells 64 --steps 20 --warmup 3 > $O/${TAG}_bench_tgv3d_n64.json 2> $O/bench_tgv.err
NSFEM_P2_ORDER=lex timeout -k 10 600 python3 bench.py --workload tgv3d-ipcs --cells 64 --steps 20 --warmup 3 > $O/${TAG}_bench_tgv3d_n64_lexicographic.json 2> $O/bench_tgv_lex.err
for o in lex morton rcm; do
  NSFEM_P2_ORDER_UNSTRUCTURED=$o timeout -k 10 600 python3 bench.py --workload dfg-bdf --steps 20 --warmup 3 > $O/${TAG}_bench_dfg_$o.json 2> $O/bench_dfg_$o.err
done
timeout -k 10 300 python3 scripts/gpu_lattice_sweep.py 512 off 0,24 0,32 1,24 > $O/${TAG}_lattice_kernel_launch_shapes_n512.txt 2>&1
timeout -k 10 300 python3 scripts/gpu_lattice_sweep.py 1024 off 0,24 0,32 > $O/${TAG}_lattice_kernel_launch_shapes_n1024.txt 2>&1
ls $O
