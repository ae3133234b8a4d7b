"""What the four pools of audio streams share on the host (sesameai-tts_amd/csrc/stream_pool.h: no HIP) as a stand-alone host program under
the host sanitizers: every single fault of a stream list and of a chunk -- a null pointer, a pool of 0 or 65 streams, 0 ids or more than
the pool has, an id of -1 or n_streams, an id twice, a negative length or offset, 2^30 + 1 samples, a stream at 2^48 -- through the plan
builders and the resets of the resampler, the stretcher, the VAD and the watermark: the exact refusal text, nothing planned, no state
moved (tools/stream_pool_check.cpp)."""
from host_check import build_and_run


def test_stream_pool_under_the_host_sanitizers(tmp_path):
    build_and_run("stream_pool_check", tmp_path, "-O1")
