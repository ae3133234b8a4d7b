"""The host plan of the limiter pool's true-peak streams and of the stateless true-peak meter (sesameai-tts_amd/csrc/limiter_plan.h: no
HIP) as a stand-alone host program under the host sanitizers: the flag's refusals, all zeros being mimi_lim_pool_reset, the emitted counts
against a walk of the definition (latency L + T), calls that mix both modes -- every output in exactly one tile, every halo inside the
stream's history and the call's LDS buffer with the signed samples T beyond it, every vector line on a 16-byte address, every gain with
exactly one source -- and every refusal with nothing planned and no state moved (tools/truepeak_plan_check.cpp)."""
from host_check import build_and_run


def test_truepeak_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("truepeak_plan_check", tmp_path, "-O1")
