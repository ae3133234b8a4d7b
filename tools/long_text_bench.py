#!/usr/bin/env python3
"""A long text on an MI355X: the sentences one after the other at B = 1, finished on the host (what ``TTS.say`` / ``export_wav`` do without
``batch=``), against the same sentences as requests of the continuously refilled batch, finished on the device
(``Generator.generate_segments``, what ``batch=`` uses).

Full-size model and codec with synthetic weights; a 190-row voice prefix (40 text rows, 149 audio rows, the EOS row) and 12 text rows per
sentence.  Synthetic weights do not reach EOS, so the workload is ragged on purpose: 64 requests with seeded per-request limits of 25 .. 125
frames, sampling 0.8 / 40, request i with seed 9000 + i.

  text      "sentence_by_sentence": per request ``TTS.generate_with_context`` with its limit (B = 1; the voice prefix's K/V is reused by
            ``Model.prefill_prompt``, as for ``say``), then the five NumPy passes of ``TTS.generate_audio_segment`` on a float32 copy.
            "live_batch_32": ONE ``generate_segments`` call at ``max_batch_size=32`` with the prefix in the prefix store.
            The two alternate round by round in one process.  wall_s: host clock from the call to the last finished segment (synchronised);
            frames_per_s: generated frames / wall_s; finish_gpu_ms: the sum over the run's ``SegmentFinisher.finish`` calls of the time between
            HIP events around each (side stream), and how many calls there were.
  finish    32 clips of 4 s already on the device: "fin_gpu_ms" between HIP events around ONE mimi_fin_segments call; "finish_wall_ms"
            ``SegmentFinisher.finish`` plus the int16 copy of every segment to the host, up to a synchronise; "host_wall_ms" per clip the float32 copy to
            the host and the five NumPy passes.  Alternating round by round.  The two are compared sample by sample: the host passes divide on the device with
            torch's tensor / scalar kernel, which multiplies by the reciprocal; the finisher divides (the rule of include/mimi_hip.h).

    python tools/long_text_bench.py --out profiles/long_text/long_text.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PREFIX, SENTENCE, REQUESTS = 190, 12, 64
TEMP, TOPK = 0.8, 40


def stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v), "n": len(v)}


def host_finish(audio: torch.Tensor, sr: int = 24000, lead_ms: int = 500, tail_ms: int = 100, fade_ms: int = 50) -> np.ndarray:
    """The finishing of ``TTS.generate_audio_segment``, pass for pass (sesameai-tts_amd/tts_service.py)."""
    audio = audio.to(torch.float32).reshape(-1)
    audio = audio / max(float(audio.abs().max()) if audio.numel() else 0.0, 1e-6)
    pcm = (audio.cpu().numpy() * 32767).astype("int16")
    pcm = np.concatenate([np.zeros(sr * lead_ms // 1000, np.int16), pcm, np.zeros(sr * tail_ms // 1000, np.int16)])
    n = min(sr * fade_ms // 1000, len(pcm) // 2)
    if n > 0:
        ramp = np.linspace(0.0, 1.0, n, dtype=np.float32)
        pcm[:n] = (pcm[:n] * ramp).astype(np.int16)
        pcm[-n:] = (pcm[-n:] * ramp[::-1]).astype(np.int16)
    return pcm


def text_leg(rounds, warmup):
    import importlib.util
    import bench
    from sesameai.finish import SegmentFinish, SegmentFinisher
    from sesameai.generator import Generator
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    spec = importlib.util.spec_from_file_location("tts_service_bench", os.path.join(ROOT, "sesameai-tts_amd", "tts_service.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)

    sd = synthetic_state_dict(csm_1b_args(), seed=1234)
    codec = MimiCodec(MimiArgs(), mimi_sd(MimiArgs(), seed=4321), max_frames=160)
    tok, msk = bench.synthetic_prompt(SimpleNamespace(ctx_text=40, ctx_frames=149, gen_text=SENTENCE), 1, 128_256, seed0=5000)
    assert tok.shape[1] == PREFIX + SENTENCE
    ctx_t, ctx_m = tok[0, :PREFIX].cuda(), msk[0, :PREFIX].cuda()
    g = torch.Generator().manual_seed(77)
    sentences = [torch.randint(0, 128_256, (SENTENCE,), generator=g).tolist() for _ in range(REQUESTS)]
    limits = [int(x) for x in torch.randint(25, 126, (REQUESTS,), generator=g)]
    seeds = [9000 + i for i in range(REQUESTS)]

    one = Generator(Model(csm_1b_args(), sd, max_frames=256, max_prefill_rows=2048), audio_tokenizer=codec, max_batch_size=1)
    tts = mod.TTS(voice_dir="/nonexistent")
    tts.generator, tts.watermarker = one, None
    tts.cached_context_tokens, tts.cached_context_masks = [ctx_t], [ctx_m]

    many = Generator(Model(csm_1b_args(), sd, max_frames=256, max_prefill_rows=2048), audio_tokenizer=codec, max_batch_size=32)
    many.cache_prefix(ctx_t, ctx_m)
    prompts = []
    for s in sentences:
        st, sm = many._tokenize_text_segment(s, 1)
        prompts.append((torch.cat([ctx_t, st], 0).long().cuda(), torch.cat([ctx_m, sm], 0).bool().cuda()))
    fin = many._finisher = SegmentFinisher("cuda")
    events = []
    plain_finish = fin.finish

    def timed_finish(clips, how, sample_rate=24000):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = plain_finish(clips, how, sample_rate); e1.record()
        events.append((e0, e1, len(clips)))
        return out
    fin.finish = timed_finish

    def sentence_by_sentence():
        one._model.seed(7)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        segs = [host_finish(tts.generate_with_context(s, 1, n * 80, TEMP, TOPK)) for s, n in zip(sentences, limits)]
        return time.perf_counter() - t0, sum((len(x) - 14400) // 1920 for x in segs)

    def live_batch():
        many._model.seed(7)
        del events[:]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        segs = many.generate_segments(prompts, limits, TEMP, TOPK, SegmentFinish(), seed=seeds)
        host = [x.cpu() for x in segs]
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return wall, sum((len(x) - 14400) // 1920 for x in host), sum(a.elapsed_time(b) for a, b, _ in events), [k for _, _, k in events]

    a_wall, a_fps, b_wall, b_fps, b_fin, b_calls = [], [], [], [], [], None
    for r in range(warmup + rounds):
        wa, fa = sentence_by_sentence()
        wb, fb, fin_ms, calls = live_batch()
        print(json.dumps({"round": r, "sentence_by_sentence_s": wa, "live_batch_32_s": wb, "frames": [fa, fb], "finish_gpu_ms": fin_ms}), flush=True)
        if r >= warmup:
            a_wall.append(wa); a_fps.append(fa / wa); b_wall.append(wb); b_fps.append(fb / wb); b_fin.append(fin_ms); b_calls = calls
    return {"requests": REQUESTS, "prefix_rows": PREFIX, "sentence_rows": SENTENCE, "limits_frames": limits, "frames_total": sum(limits),
            "sampling": [TEMP, TOPK],
            "sentence_by_sentence": {"wall_s": stats(a_wall), "frames_per_s": stats(a_fps)},
            "live_batch_32": {"wall_s": stats(b_wall), "frames_per_s": stats(b_fps), "finish_gpu_ms_per_run": stats(b_fin),
                              "finish_calls_last_run": len(b_calls), "clips_per_finish_call_last_run": b_calls},
            "wall_ratio_median": statistics.median(a_wall) / statistics.median(b_wall)}


def finish_leg(rounds, warmup):
    from sesameai import _abi
    from sesameai.finish import SegmentFinish, SegmentFinisher
    N, n = 32, 4 * 24000
    fin = SegmentFinisher("cuda")
    clips = [(torch.randn(n, generator=torch.Generator().manual_seed(300 + i)) * 0.2).cuda() for i in range(N)]
    ptrs = (C.c_void_p * N)(*[c.data_ptr() for c in clips])
    lens, lead, tail, fade = (C.c_long * N)(*[n] * N), (C.c_int32 * N)(*[12000] * N), (C.c_int32 * N)(*[2400] * N), (C.c_int32 * N)(*[1200] * N)
    off, n_out = (C.c_long * N)(), (C.c_long * N)()
    out = torch.empty(N * (n + 14400), dtype=torch.int16, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def gpu():
        e0.record()
        rc = _abi.lib.mimi_fin_segments(fin._h, ptrs, lens, lead, tail, fade, N, out.data_ptr(), off, n_out, torch.cuda.current_stream().cuda_stream)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    t_gpu, t_dev, t_host = [], [], []
    differ, worst = 0, 0
    for r in range(warmup + rounds):
        a = gpu()
        b, dev = wall(lambda: [y.cpu().numpy() for y in fin.finish(clips, SegmentFinish())])
        c, host = wall(lambda: [host_finish(x) for x in clips])
        # (the host passes divide ON THE DEVICE, as generate_audio_segment does with a device clip: torch's device kernel for tensor / scalar
        #  multiplies by the reciprocal, the finisher divides -- the two may differ by one LSB in a few samples)
        d = [np.abs(x.astype(np.int32) - y.astype(np.int32)) for x, y in zip(dev, host)]
        differ, worst = sum(int((x != 0).sum()) for x in d), max(int(x.max()) for x in d)
        if r >= warmup:
            t_gpu.append(a); t_dev.append(b); t_host.append(c)
    return {"clips": N, "seconds_per_clip": 4, "fin_gpu_ms": stats(t_gpu), "finish_wall_ms": stats(t_dev), "host_wall_ms": stats(t_host),
            "host_over_finish_wall": statistics.median(t_host) / statistics.median(t_dev),
            "samples": N * (n + 14400), "samples_that_differ_from_the_host_passes": differ, "largest_difference_lsb": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--finish-rounds", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("long_text_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/long_text_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "wall: host clock up to a synchronise; gpu_ms: between HIP events; statistics over alternating rounds", "rounds": args.rounds, "warmup": args.warmup}
    res["finish"] = finish_leg(args.finish_rounds, 3)
    print(json.dumps({"finish": res["finish"]}), flush=True)
    res["text"] = text_leg(args.rounds, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
