"""The segment plan of a pool of Mimi encode streams (sesameai-tts_amd/csrc/enc_stream_segs.h: no HIP) as a stand-alone host program under
the host sanitizers: every refusal of mimi_enc_pool_encode, the prefix sums and the frame -> segment map, every level's rows of a last
partial frame against enc_level_len of the chunk's own samples, and the 2^31-token bound (tools/enc_stream_segs_check.cpp)."""
from host_check import build_and_run


def test_enc_stream_segs_under_the_host_sanitizers(tmp_path):
    build_and_run("enc_stream_segs_check", tmp_path, "-O1")
