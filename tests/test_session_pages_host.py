"""The page bookkeeping of the session store (sesameai-tts_amd/csrc/session_pages.h: no HIP) as a stand-alone host program: a pool too short
for a grow leaves the session as it was, after any interleaving of grow / truncate / close every page is owned exactly once or is free, and
the copy plans cover their row ranges (ending on a page boundary, one past it, starting mid-page, a single row)."""
from host_check import build_and_run


def test_session_pages_under_the_host_sanitizers(tmp_path):
    build_and_run("session_pages_check", tmp_path)
