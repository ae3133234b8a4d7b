"""Times the device's Whisper encoder (sesameai/whisper_enc.py) by HIP events around ``encode``: median and min .. max of ``--iters`` calls
after ``--warmup``, seeded random weights (tests/whisper_enc_ref.make_weights), at the shapes the reference's chat runs -- d = 768 / L = 12,
d = 1024 / L = 24 (distil-medium.en), d = 1280 / L = 32 / 128 mels (distil-large-v3) -- each at B = 1 and B = 4.  Where transformers imports,
``model.get_encoder()`` of the same config in fp16 is timed on the same box, after ours, the same way.  The END-of-turn chain is one number
more: the turn's last MelPool feed + finish + encode at distil-medium, B = 1.  The FLOP of an encode are counted from the shapes (GEMMs,
convolutions and attention's two products); "of peak" is that over the time over the 2.5 PFLOP/s dense fp16 matrix peak: a whole-encode rate,
not a kernel's.  Per-kernel times come from a profiler run of this script with ``--only medium --batches 1 --no-hf``.  One JSON line.
  python tools/whisper_enc_bench.py [--iters 30] [--warmup 5] [--only small,medium,large] [--batches 1,4] [--no-hf] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sesameai-tts_amd"), os.path.join(ROOT, "tests")]

PEAK_F16_MFMA = 2.5e15            # FLOP/s, dense fp16 on the matrix cores
SHAPES = {
    "small": dict(n_mels=80, d_model=768, n_layers=12, n_heads=12, ffn_dim=3072, n_ctx=1500, ln_eps=1e-5),
    "medium": dict(n_mels=80, d_model=1024, n_layers=24, n_heads=16, ffn_dim=4096, n_ctx=1500, ln_eps=1e-5),
    "large": dict(n_mels=128, d_model=1280, n_layers=32, n_heads=20, ffn_dim=5120, n_ctx=1500, ln_eps=1e-5),
}


def encode_flop(c, batch):
    T, d, f = c["n_ctx"], c["d_model"], c["ffn_dim"]
    conv = 2 * (2 * T) * d * 3 * c["n_mels"] + 2 * T * d * 3 * d
    layer = 2 * T * d * (3 * d) + 2 * T * d * d + 2 * 2 * T * d * f + 2 * 2 * T * T * d
    return batch * (conv + c["n_layers"] * layer)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="small,medium,large")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import whisper_enc_ref as R
    from sesameai.whisper_enc import WhisperEncoder
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    dev = torch.device("cuda")
    batches = [int(b) for b in args.batches.split(",")]
    res = {"peak_f16_flops": PEAK_F16_MFMA, "shapes": {}}
    for name in args.only.split(","):
        cfg = SHAPES[name]
        sd = R.make_weights(cfg, 1, 1.0)
        enc = WhisperEncoder(cfg, sd, max_batch=max(batches))
        entry = {"config": cfg, "plan_b1": enc.describe(1)}
        feats = torch.stack([R.make_features(cfg["n_mels"], 2 * cfg["n_ctx"], 10 + k, 600 + 300 * k) for k in range(max(batches))]).to(dev)
        for b in batches:
            t = timed(lambda: enc.encode(feats[:b], dtype=torch.float16), args.iters, args.warmup)
            t["flop"] = encode_flop(cfg, b)
            t["tflops"] = t["flop"] / (t["median_ms"] * 1e-3) / 1e12
            t["of_peak"] = t["tflops"] * 1e12 / PEAK_F16_MFMA
            entry[f"ours_b{b}"] = t
        if name == "medium":                                   # the END-of-turn chain: last feed + finish + encode, one stream, a 10 s turn
            import mel_ref as M
            from sesameai.mel import MelPool
            pool = MelPool(1, cfg["n_mels"], device=dev)
            speech = torch.from_numpy(M.signal("speech", 7, 160000)).to(dev)
            held, ms = {}, []
            for k in range(args.warmup + args.iters):
                pool.reset([0])
                held["rows"] = pool.feed([0], [speech[:160000 - 1280]], False)[0].clone()
                torch.cuda.synchronize()
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                (rows,) = pool.feed([0], [speech[160000 - 1280:]], True)
                enc.encode(pool.finish([torch.cat([held["rows"], rows])])[0], dtype=torch.float16)
                z.record()
                z.synchronize()
                if k >= args.warmup:
                    ms.append(a.elapsed_time(z))
            entry["end_of_turn_chain_b1"] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iters": args.iters}
        del enc
        if not args.no_hf:
            try:
                from transformers import WhisperConfig, WhisperForConditionalGeneration
                model = WhisperForConditionalGeneration(WhisperConfig(**R.hf_config(cfg))).eval()
                hf = model.get_encoder()
                hf.load_state_dict(sd)
                hf = hf.to(dev, torch.float16)
                entry["hf_attn_implementation"] = str(getattr(model.config, "_attn_implementation", "?"))
                with torch.inference_mode():
                    for b in batches:
                        x16 = feats[:b].half()
                        entry[f"hf_fp16_b{b}"] = timed(lambda: hf(x16).last_hidden_state, args.iters, args.warmup)
                del hf, model
            except ImportError as e:                           # transformers absent: the comparison is not taken here
                entry["hf_skipped"] = f"{type(e).__name__}: {e}"
        res["shapes"][name] = entry
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
