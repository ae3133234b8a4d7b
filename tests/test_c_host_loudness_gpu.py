"""examples/c_host/mimi_c_host.c, the loudness half: from plain C the decoded clip goes through mimi_ld_pool_feed / mimi_ld_pool_integrate
and mimi_fin_segments_ld on one stream.  The meter's row it prints and the int16 segment it writes are those of the Python host
(sesameai/loudness.py, sesameai/finish.py) and of the rule (tests/loudness_ref.py) for the same PCM."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import loudness_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIMI_HOST = os.path.join(ROOT, "examples", "c_host", "mimi_c_host")


def test_plain_c_meters_and_finishes_like_the_python_host(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(MIMI_HOST):
        r = subprocess.run(["make", "-C", os.path.dirname(MIMI_HOST)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    from sesameai.finish import SegmentFinish, SegmentFinisher
    from sesameai.loudness import measure
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(mimi_tiny_args(), seed=4321)
    codec = MimiCodec(mimi_tiny_args(), sd, max_frames=16)
    n0 = len(codec._keep)
    cfg, w = codec._build(sd)                                      # a second image of the structs, with the tensors behind it in _keep[n0:]
    tensors = codec._keep[n0:]
    T = 10
    codes = torch.randint(0, 2048, (1, 32, T), generator=torch.Generator().manual_seed(31))
    blob, out, seg = str(tmp_path / "codec.blob"), str(tmp_path / "out.pcm"), str(tmp_path / "seg.i16")
    with open(blob, "wb") as f:
        f.write(b"MIMB")
        f.write(struct.pack("<ii", C.sizeof(cfg), C.sizeof(w)))
        f.write(bytes(cfg)); f.write(bytes(w))
        f.write(struct.pack("<i", len(tensors)))
        for t in tensors:
            b = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            f.write(struct.pack("<Qq", t.data_ptr(), len(b))); f.write(b)
        f.write(struct.pack("<i", T))
        f.write(codes[0].to(torch.int32).contiguous().numpy().tobytes())
    pcm = codec.decode(codes)[0, 0]
    r = subprocess.run([MIMI_HOST, blob, out, seg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"loudness: S (-?\d+) n (-?\d+) peak (-?\d+) hops (-?\d+); finished (\d+) samples", r.stdout)
    assert m, r.stdout[-2000:]
    row = tuple(int(v) for v in m.groups()[:4])
    x = pcm.cpu().numpy()
    assert row == L.measure_ref(x) == tuple(measure([pcm])[0]) and row[3] == x.shape[0] // L.H == 8
    got = np.fromfile(seg, dtype=np.int16)
    how = SegmentFinish(0, 0, 0, loudness=-19.0, ceiling_db=-1.0)
    assert how.level() == (15848927, 29203)                        # the integers the C host passes
    assert np.array_equal(got, SegmentFinisher().finish([pcm], how)[0].cpu().numpy())
    assert np.array_equal(got, L.finish_ld_ref(x, 0, 0, 0, *how.level()))
