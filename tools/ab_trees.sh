# ab_trees.sh DIR [MODE ...] : interleaved same-box A/B of two checked-out trees (DIR = an older commit's tree with its own built library, this tree = new):
#   git worktree add -f _old <commit>; (cd _old && python -m transformer4sed_amd.build); gpurun -- 'bash tools/ab_trees.sh _old'
# Without modes: three pairs of finetune2, two of pretrain and of finetune1.  With modes (any of bench.py --mode): three pairs of each.
# Every bench run has its own time limit; the first one that fails or runs into it ends the script (nothing more is started on the GPU).
set -o pipefail
run() { (cd "$1" && timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 10 --mode "$2" 2>/dev/null | tail -1 | python -c "import sys, json; d = json.loads(sys.stdin.read()); r = d.get('roofline') or {}; h = d.get('host') or {}; print(d['value'], 'clips/s', d['ms_per_step'], 'ms  cpu_ms_per_step', h.get('cpu_ms_per_step'), ' issue_ms_per_step', h.get('issue_ms_per_step'), ' GEMM family', r.get('achieved'), 'TFLOP/s')"); }
line() { out=$(run "$2" "$3") || { echo "$1 $3: bench run failed, stopping"; exit 1; }; echo "$1 $3: $out"; }
pairs() { for r in $(seq "$2"); do line old "$old" "$1"; line new . "$1"; done; }
old=$1; shift
if [ $# -eq 0 ]; then
  pairs finetune2 3; pairs pretrain 2; pairs finetune1 2
else
  for m in "$@"; do pairs "$m" 3; done
fi
