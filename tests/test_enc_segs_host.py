"""The clip plan of a ragged Mimi encode (sesameai-tts_amd/csrc/enc_segs.h: no HIP) as a stand-alone host program under the host
sanitizers: for every list of up to four clips around the seams (1, hop / 2, hop +- 1, 2 hop +- 1 samples) the slots do not overlap, the
rows fit them, every level's row count is the single encode's, and every refusal of mimi_encode_many is made (tools/enc_segs_check.cpp)."""
from host_check import build_and_run


def test_enc_segs_under_the_host_sanitizers(tmp_path):
    build_and_run("enc_segs_check", tmp_path, "-O1")
