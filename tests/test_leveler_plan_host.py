"""The host plan of the live leveler (sesameai-tts_amd/csrc/loudness_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: the parameter ranges of mimi_ld_pool_level_reset at both ends, the mode refusals of the metering feed, the leveler's feed
and the state read with nothing planned and no state moved, the refusals of `out` and `gain`, the packed gain offsets, and the apply
plan walked the way k_ld_apply walks it over a sweep of lengths, offsets, formats and buffer phases -- every sample in exactly one line,
every vector line inside its chunk and on a 16-byte address, every gain index inside the stream's values (tools/leveler_plan_check.cpp)."""
from host_check import build_and_run


def test_leveler_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("leveler_plan_check", tmp_path, "-O1")
