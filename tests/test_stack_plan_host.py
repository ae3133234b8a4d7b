"""The launch plan of a transformer layer (sesameai-tts_amd/csrc/stack_plan.h: no HIP) as a stand-alone host program.  The wide-M kernel
families are bit-identical to one another, so the parity tests cannot see a call that takes another kernel than it did; the program pins
which family, split and activation order every listed call chooses, and which public ``kind`` numbers ``csm_op_gemv`` accepts."""
import os
import shutil
import subprocess


def test_stack_plan_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "stack_plan_check")
    r = subprocess.run([hipcc, "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "stack_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr, r.stdout + r.stderr
