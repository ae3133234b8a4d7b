"""The host plan of the segment finisher (sesameai-tts_amd/csrc/finish_plan.h: no HIP) as a stand-alone host program under the host sanitizers:
every refusal of mimi_fin_segments, the packed output offsets (odd ones, and an odd buffer address), the tile counts of both kernels at
lengths around one tile and up to 2^30 samples, 64 segments, N = 0, and every block of a plan walked the way the kernels walk it
(tools/finish_plan_check.cpp)."""
import os
import shutil
import subprocess


def test_finish_plan_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "finish_plan_check")
    r = subprocess.run([hipcc, "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "finish_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
