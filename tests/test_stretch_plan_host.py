"""The host plan of a pool of time-stretch streams (sesameai-tts_amd/csrc/stretch_plan.h: no HIP) as a stand-alone host program under the host
sanitizers: every refusal of mimi_ts_pool_reset / mimi_ts_pool_feed, the packed output and block offsets, the emitted counts against the
definition for nine speeds, the carry bound, and a stream walked past 2^40 samples whose kernel-visible numbers stay relative to the carry's
base (tools/stretch_plan_check.cpp)."""
import os
import shutil
import subprocess


def test_stretch_plan_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "stretch_plan_check")
    r = subprocess.run([hipcc, "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "stretch_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
