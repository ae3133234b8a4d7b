# ms per frame step (B = 1) and the two dominant kernels' live timings for alternative builds of the library (CSM_HIP_LIB)
cd "$(dirname "$0")/../.."
for lib in "$@"; do
  echo -n "$lib: "
  CSM_HIP_LIB=$PWD/sesameai-tts_amd/lib/$lib timeout 300 python bench.py --steps 100 --warmup 10 --no-cpu-baseline --no-mimi --no-extras --full 2>/dev/null | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); k=d['roofline']['dominant_kernels']; print(d['ms_per_step'], [(x['kernel'], x['avg_us']) for x in k])"
done
