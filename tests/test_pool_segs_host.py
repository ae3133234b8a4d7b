"""The segment plan of a ragged stream-pool decode (sesameai-tts_amd/csrc/pool_segs.h: no HIP) as a stand-alone host program under the host
sanitizers: for every list of up to four segments with T_i in {1, 2, max - 1, max} the dense slots tile [0, R * F) at every level without
gap or overlap, frame_seg is right at every frame, and every refusal of mimi_pool_decode_ragged is made (tools/pool_segs_check.cpp)."""
from host_check import build_and_run


def test_pool_segs_under_the_host_sanitizers(tmp_path):
    build_and_run("pool_segs_check", tmp_path, "-O1")
