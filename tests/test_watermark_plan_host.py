"""The host plan of the keyed watermark pool (sesameai-tts_amd/csrc/watermark_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: every refusal of mimi_wm_pool_reset / mimi_wm_pool_feed / mimi_wm_pool_detect at both sides of both ends of its range with
nothing planned and no state moved, the output counts against the definition, the carry that never reaches 1920 samples, the packed
places, and a stream walked past 2^40 samples whose kernel-visible numbers stay small (tools/wm_plan_check.cpp)."""
from host_check import build_and_run


def test_watermark_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("wm_plan_check", tmp_path, "-O1")
