"""SessionPages::forget (sesameai-tts_amd/csrc/session_pages.h: no HIP) as a stand-alone host program under the address and undefined-behaviour
sanitizers: a forget the pool is too short for leaves the session and the free list as they were; over 4,000 seeded steps of grow /
truncate / forget / close / open on six sessions and 23 pages every page is owned by exactly one session or is free; and the page lists and
plans after a forget are right for from page-aligned, not page-aligned, from and to in one page, a tail that ends mid-page, to == rows,
from == 0 and a single row (tools/session_forget_check.cpp)."""
from host_check import build_and_run


def test_session_forget_under_the_host_sanitizers(tmp_path):
    build_and_run("session_forget_check", tmp_path)
