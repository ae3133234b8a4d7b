"""The segment plan of a pool of Mimi encode streams (sesameai-tts_amd/csrc/enc_stream_segs.h: no HIP) as a stand-alone host program under
the host sanitizers: every refusal of mimi_enc_pool_encode, the prefix sums and the frame -> segment map, every level's rows of a last
partial frame against enc_level_len of the chunk's own samples, and the 2^31-token bound (tools/enc_stream_segs_check.cpp)."""
import os
import shutil
import subprocess


def test_enc_stream_segs_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "enc_stream_segs_check")
    r = subprocess.run([hipcc, "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "enc_stream_segs_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
