"""The page bookkeeping of the session store (sesameai-tts_amd/csrc/session_pages.h: no HIP) as a stand-alone host program: a pool too short
for a grow leaves the session as it was, after any interleaving of grow / truncate / close every page is owned exactly once or is free, and
the copy plans cover their row ranges (ending on a page boundary, one past it, starting mid-page, a single row)."""
import os
import shutil
import subprocess


def test_session_pages_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "session_pages_check")
    r = subprocess.run([hipcc, "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "session_pages_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
