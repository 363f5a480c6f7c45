cd "$(dirname "$0")/.."
O=${1:-bench_out}
mkdir -p $O
python -m pytest tests -q -m gpu --tb=short 2>&1 | tail -25 > $O/r04_gpu_suite.log
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/r04_bench_driver_cmd.json 2> $O/r04_bench.err
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/r04_bench_driver_cmd_2.json 2>> $O/r04_bench.err
VFN_WINOGRAD=0 python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > $O/r04_bench_driver_cmd_winograd_off.json 2>> $O/r04_bench.err
python bench.py --full > $O/r04_bench_default.json 2>> $O/r04_bench.err
VFN_DIST_BACKEND=gloo VFN_SINGLE_DEVICE=1 python bench.py --full --gpus 2 --steps 20 --warmup 5 --no-cpu-baseline > $O/r04_bench_2ranks_one_device_gloo.json 2>> $O/r04_bench.err
python bench.py --full --workload C3 --precision bf16x3 --no-cpu-baseline > $O/r04_bench_c3_bf16x3.json 2>> $O/r04_bench.err
python bench.py --full --workload C3 --precision bf16 --no-cpu-baseline > $O/r04_bench_c3_bf16.json 2>> $O/r04_bench.err
python scripts/bench_train_step.py 6 400 400 2 8 > $O/r04_train_step.txt 2>&1
python scripts/bench_train_step.py 6 400 400 2 8 >> $O/r04_train_step.txt 2>&1
bash scripts/profile_train.sh r04
python scripts/profile_round.py fp32 > $O/r04_profile_round.log 2>&1
python scripts/profile_layers.py > $O/r04_layers.txt 2>&1
