"""The owner of a CSM handle's device memory (sesameai-tts_amd/csrc/dev_pool.h: no HIP) as a stand-alone host program against a counting
fake backend: with any one allocation or fill refused, everything the backend handed out is freed exactly once and nothing else is."""
from host_check import build_and_run


def test_dev_pool_under_the_host_sanitizers(tmp_path):
    build_and_run("dev_pool_check", tmp_path)
