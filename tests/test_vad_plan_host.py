"""The host plan of a pool of voice-activity streams (sesameai-tts_amd/csrc/vad_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: every refusal of mimi_vad_pool_reset / mimi_vad_pool_feed with nothing planned and no state moved, the packed frame offsets,
the frame counts against the definition, the carry bound of 879 samples, and a stream walked past 2^40 samples whose kernel-visible numbers
stay relative to the carry's base (tools/vad_plan_check.cpp)."""
from host_check import build_and_run


def test_vad_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("vad_plan_check", tmp_path, "-O1")
