"""The host plan of the segment finisher (sesameai-tts_amd/csrc/finish_plan.h: no HIP) as a stand-alone host program under the host sanitizers:
every refusal of mimi_fin_segments, the packed output offsets (odd ones, and an odd buffer address), the tile counts of both kernels at
lengths around one tile and up to 2^30 samples, 64 segments, N = 0, and every block of a plan walked the way the kernels walk it
(tools/finish_plan_check.cpp)."""
from host_check import build_and_run


def test_finish_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("finish_plan_check", tmp_path, "-O1")
