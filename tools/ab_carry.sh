# A/B of MVD_NO_CARRY=1 against MVD_DUMMY=1 (the default path) on ONE box: bash tools/ab_carry.sh <outdir>
O=${1:?usage: bash tools/ab_carry.sh <outdir>}; mkdir -p $O
timeout 1500 python -m pytest tests/test_gpu_model.py tests/test_gpu_determinism.py tests/test_gpu_variants.py -m gpu -q -s -k "blocks or unet_small or unet_full or step_full or bit_reproducible or variant or trajectory" 2>&1 | grep -E "parity|property|passed|failed|Error|error|assert|FAILED|^E " | tail -40 > $O/pytest.log
tail -40 $O/pytest.log
for v in MVD_NO_CARRY=1 MVD_DUMMY=1 MVD_NO_CARRY=1 MVD_DUMMY=1; do env $v timeout 300 python bench.py --steps 30 --warmup 5 --full --no-cpu-baseline --no-extras 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$v', round(d['ms_per_step'],3), 'ms', sum(f['launches_per_step'] for f in d['families']))"; done | tee $O/ab_carry.txt
for v in MVD_NO_CARRY=1 MVD_DUMMY=1; do env $v timeout 300 python bench.py --steps 30 --warmup 5 --no-cpu-baseline --no-extras --simulate-gpus 8 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('sim8 $v', round(d['ms_per_step'],3), 'ms')"; done | tee -a $O/ab_carry.txt
