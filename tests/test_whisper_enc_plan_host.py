"""The host plan of the Whisper encoder (sesameai-tts_amd/csrc/whisper_enc_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: every refusal of a config, the tile choice around the 256-workgroup threshold, and the launch list of an encode -- 2 + 7 L + 1
launches whose workgroups cover M and N with their tails -- for every Whisper size at batches 1 .. 64 (tools/whisper_enc_plan_check.cpp)."""
from host_check import build_and_run


def test_whisper_enc_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("whisper_enc_plan_check", tmp_path, "-O1")
