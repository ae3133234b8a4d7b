"""SessionPages::forget (sesameai-tts_amd/csrc/session_pages.h: no HIP) as a stand-alone host program under the address and undefined-behaviour
sanitizers: a forget the pool is too short for leaves the session and the free list as they were; over 4,000 seeded steps of grow /
truncate / forget / close / open on six sessions and 23 pages every page is owned by exactly one session or is free; and the page lists and
plans after a forget are right for from page-aligned, not page-aligned, from and to in one page, a tail that ends mid-page, to == rows,
from == 0 and a single row (tools/session_forget_check.cpp)."""
import os
import shutil
import subprocess


def test_session_forget_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "session_forget_check")
    r = subprocess.run([hipcc, "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "session_forget_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
