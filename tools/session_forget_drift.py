#!/usr/bin/env python3
"""How far a key drifts that survives many forgets (CPU only; recorded in docs/experiments/session_forget.md, not gated).

A kept row is rotated back once per forget and rounded to bf16 each time.  256 unrotated keys (head_dim 64, N(0, 1), rounded to bf16) are
rotated to position 1,800 as the prompt kernels do (the bf16 rope table, fp32 arithmetic, one rounding), then forgotten 16 times in
succession by d = 100 rows each -- csm_session_forget's arithmetic: fp32 on the bf16 values, separate multiplies and adds, one rounding --
and compared with the SAME unrotated key rotated once to its final position 200 in float64.  Two rotation tables are compared:

  fp32   (cos, sin)(d theta) computed in float64 and rounded to float: what ``Session.forget`` hands the kernel
  bf16   the model's bf16 rope table at index d: what a kernel that reused the table would use (2^-9 relative error per entry, the same
         error at every forget, so it accumulates linearly)

and, for scale, the error of a key written at position 200 directly (the table's own error and one rounding).  Relative error = |k - ref|_2 /
|ref|_2 per key; mean and maximum over the keys.

    python tools/session_forget_drift.py --out profiles/session_forget/drift.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

P0, D, TIMES, KEYS = 1800, 100, 16, 256


def rotate(x, c, s, back):
    """Interleaved pairs of x (n, hd) bf16 by (c, s) (hd / 2,) fp32; fp32 arithmetic, one rounding to bf16."""
    v = x.float().unflatten(-1, (-1, 2))
    x0, x1 = v[..., 0], v[..., 1]
    o = [x0 * c + x1 * s, x1 * c - x0 * s] if back else [x0 * c - x1 * s, x1 * c + x0 * s]
    return torch.stack(o, dim=-1).flatten(-2).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sesameai.models import FLAVORS, llama3_rope_table, llama3_rope_theta
    f = FLAVORS["llama-1B"]
    theta, table = llama3_rope_theta(f).double(), llama3_rope_table(f).float()
    keys = torch.randn(KEYS, f.head_dim, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    final = P0 - TIMES * D
    v = keys.double().unflatten(-1, (-1, 2))

    def rel(k, pos):
        ang = pos * theta
        ref = torch.stack([v[..., 0] * torch.cos(ang) - v[..., 1] * torch.sin(ang), v[..., 1] * torch.cos(ang) + v[..., 0] * torch.sin(ang)], dim=-1).flatten(-2)
        return (k.double() - ref).norm(dim=-1) / ref.norm(dim=-1)
    rots = {"fp32": (torch.cos(D * theta).float(), torch.sin(D * theta).float()), "bf16_table": (table[D, :, 0], table[D, :, 1])}
    res = dict(head_dim=f.head_dim, keys=KEYS, start_position=P0, rows_per_forget=D, forgets=TIMES, final_position=final)
    direct = rotate(keys, table[final, :, 0], table[final, :, 1], back=False)
    res["written_at_final_position_directly"] = dict(mean=float(rel(direct, final).mean()), max=float(rel(direct, final).max()))
    for name, (c, s) in rots.items():
        k = rotate(keys, table[P0, :, 0], table[P0, :, 1], back=False)
        curve = []
        for i in range(TIMES):
            k = rotate(k, c, s, back=True)
            curve.append(round(float(rel(k, P0 - (i + 1) * D).mean()), 6))
        res[name] = dict(mean=float(rel(k, final).mean()), max=float(rel(k, final).max()), mean_after_each_forget=curve)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
