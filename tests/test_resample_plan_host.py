"""The host plan of a pool of resampler streams (sesameai-tts_amd/csrc/resample_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: every refusal of mimi_rs_pool_create / mimi_rs_pool_feed, the packed output offsets, the emitted counts against the formula for
the ten rate pairs, and a stream walked past 2^40 samples whose kernel-visible numbers stay those of its totals reduced by whole periods
(tools/resample_plan_check.cpp)."""
from host_check import build_and_run


def test_resample_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("resample_plan_check", tmp_path, "-O1")
