"""The owner of a CSM handle's device memory (sesameai-tts_amd/csrc/dev_pool.h: no HIP) as a stand-alone host program against a counting
fake backend: with any one allocation or fill refused, everything the backend handed out is freed exactly once and nothing else is."""
import os
import shutil
import subprocess


def test_dev_pool_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "dev_pool_check")
    r = subprocess.run([hipcc, "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "dev_pool_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
