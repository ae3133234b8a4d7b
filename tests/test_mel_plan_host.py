"""The host plan of the log-mel pool (sesameai-tts_amd/csrc/mel_plan.h: no HIP) as a stand-alone host program under the host sanitizers:
every refusal of the spine through mel_plan_build and mel_reset with nothing planned and no state moved, the frame counts around 200,
201, 360, 361, the cap and `final` against a walk of the definition, the dropped count past the cap, carry lengths, packed row offsets,
and a host walk of the two kernels' index arithmetic over chunk schedules (tools/mel_plan_check.cpp)."""
from host_check import build_and_run


def test_mel_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("mel_plan_check", tmp_path, "-O1")
