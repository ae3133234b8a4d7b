"""The host plan of a pool of time-stretch streams (sesameai-tts_amd/csrc/stretch_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: every refusal of mimi_ts_pool_reset / mimi_ts_pool_feed, the packed output and block offsets, the emitted counts against the
definition for nine speeds, the carry bound, and a stream walked past 2^40 samples whose kernel-visible numbers stay relative to the carry's
base (tools/stretch_plan_check.cpp)."""
from host_check import build_and_run


def test_stretch_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("stretch_plan_check", tmp_path, "-O1")
