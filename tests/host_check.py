"""The stand-alone host checks under tools/: plain C++ programs with their own ``main`` that drive the headers of sesameai-tts_amd/csrc
which hold no HIP, built with the address and undefined-behaviour sanitizers on the host side and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(name, tmp_path, opt=None):
    """Compile tools/``name``.cpp under the host sanitizers (``opt``: its optimisation flag, e.g. "-O1") and run it: it must exit 0,
    print ``ok`` and leave stderr empty."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / name)
    r = subprocess.run([hipcc, "-std=c++17"] + ([opt] if opt else []) +
                       ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "sesameai-tts_amd", "csrc"), os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
