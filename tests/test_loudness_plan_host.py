"""The host plan of a pool of loudness-meter streams (sesameai-tts_amd/csrc/loudness_plan.h: no HIP) as a stand-alone host program under the
host sanitizers: every refusal of mimi_ld_pool_create / reset / feed / integrate and of mimi_fin_segments_ld's own arguments with nothing
planned and no state moved, the shared spine's texts byte for byte, the packed hop offsets, the hop counts and carry lengths over a sweep
of R around the multiples of H, that `final` leaves the stream fresh, and a stream walked past 2^40 samples whose kernel-visible numbers
stay relative to the carry's base (tools/loudness_plan_check.cpp)."""
from host_check import build_and_run


def test_loudness_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("loudness_plan_check", tmp_path, "-O1")
