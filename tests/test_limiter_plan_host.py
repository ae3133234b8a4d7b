"""The host plan of the look-ahead limiter pool (sesameai-tts_amd/csrc/limiter_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: the parameter ranges of mimi_lim_pool_reset at both ends, every refusal of reset, feed and state with nothing planned and no
state moved, the emitted counts against a walk of the definition, and the tile plan -- every output in exactly one tile, every halo inside
the stream's history and the call's LDS buffer, every vector line on a 16-byte address (tools/limiter_plan_check.cpp)."""
from host_check import build_and_run


def test_limiter_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("limiter_plan_check", tmp_path, "-O1")
