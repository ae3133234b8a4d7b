"""The device voice-activity pool (include/mimi_hip.h mimi_vad_pool_*, sesameai/vad.py) against the rule (tests/vad_ref.py): every check is
np.array_equal on flags, lag, power, floor and the summary -- one-shot, streamed over the oracle test's schedules, fp32 and int16, in any
company, order and stream id, after final, on the inputs where each part of the rule is decisive, and with parameters at their bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import vad_ref as V
from test_vad_oracle import LENGTHS, QUICK, clip, full_scale_square, noise, pulses, ref, schedules, talk, voice

pytestmark = pytest.mark.gpu
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pool(n=64):
    from sesameai.vad import VadPool
    if ("pool", n) not in _cache:
        _cache[("pool", n)] = VadPool(n)
    return _cache[("pool", n)]


def _prm(p):
    from sesameai.vad import VadParams
    return VadParams(*p)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _same(fr, want, what, summary=None):
    for f in ("flags", "lag", "power", "floor"):
        got, w = getattr(fr, f).cpu().numpy(), getattr(want, f)
        assert got.dtype == w.dtype and got.shape == w.shape, (what, f, got.shape, w.shape)
        assert np.array_equal(got, w), (what, f, int(np.count_nonzero(got != w)), np.flatnonzero(got != w)[:5].tolist())
    if summary is not None:
        assert list(summary) == [bool(want.summary[0])] + want.summary[1:7].tolist(), (what, "summary", summary, want.summary.tolist())


def _cat(frs):
    from sesameai.vad import VadFrames
    return VadFrames(*(torch.cat([getattr(f, n) for f in frs]) for n in ("flags", "lag", "power", "floor")), frs[0].first)


def _streamed(pool, ids, prms, clips, scheds):
    """Every clip through its own stream on its own schedule, all streams sharing the calls: step t feeds every stream that still has a
    chunk; what is left of a clip (maybe nothing) goes with final.  frame_count and the frames' first index are checked at every feed.
    -> per stream its frames, concatenated, and its summary after its final call."""
    pool.reset(ids, [_prm(p) for p in prms])
    clips = [_t(c).cuda() for c in clips]
    cuts = [V.cut(c.shape[0], s) for c, s in zip(clips, scheds)]
    out, seen, summ = [[] for _ in ids], [0] * len(ids), [None] * len(ids)
    for t in range(max(len(p) for p, _ in cuts) + 1):
        live = [j for j in range(len(ids)) if t <= len(cuts[j][0])]
        fin = [t == len(cuts[j][0]) for j in live]
        chunks = [clips[j][cuts[j][1]:] if f else clips[j][cuts[j][0][t][0]:cuts[j][0][t][1]] for j, f in zip(live, fin)]
        counts = [pool.frame_count(ids[j], c.shape[0], f) for j, c, f in zip(live, chunks, fin)]
        frs = pool.feed([ids[j] for j in live], chunks, fin)
        assert [int(f.flags.shape[0]) for f in frs] == counts
        polled = pool.poll() if any(fin) else None
        for j, fr, f in zip(live, frs, fin):
            assert fr.first == seen[j]
            seen[j] += int(fr.flags.shape[0])
            out[j].append(fr)
            if f:
                summ[j] = polled[ids[j]]
    return [_cat(v) for v in out], summ


def test_one_stream_over_the_lengths_and_schedules_is_the_rule():
    _need_gpu()
    pool = _pool()
    jobs = [(N, name, sch) for N in LENGTHS for name, sch in schedules(N, N + 1).items()]
    ids = list(range(len(jobs)))
    frs, summ = _streamed(pool, ids, [QUICK] * len(jobs), [clip(N) for N, _, _ in jobs], [sch for _, _, sch in jobs])
    from sesameai.vad import events
    for (N, name, _), fr, sm in zip(jobs, frs, summ):
        _same(fr, ref(N), (N, name), sm)
        assert events(fr, _prm(QUICK)) == ref(N).events


def test_fp32_and_int16_of_the_same_clip():
    _need_gpu()
    from sesameai.vad import detect
    x = clip(24000)
    i16 = V.to_s(x).astype(np.int16)
    frs, summ = detect([_t(x), _t(i16).cuda()], _prm(QUICK), want_summary=True)           # mixed: the int16 clip goes as fp32, exactly
    _same(frs[0], ref(24000), "fp32", summ[0]); _same(frs[1], ref(24000), "int16 among fp32", summ[1])
    frs = detect([_t(i16), _t(i16[:5000]).cuda()], _prm(QUICK))                           # all int16: the int16 path of the kernels
    _same(frs[0], ref(24000), "int16")
    _same(frs[1], V.vad_ref(x[:5000], QUICK), "int16, short")
    pool = _pool()
    frs, summ = _streamed(pool, [4], [QUICK], [i16], [schedules(24000, 1)["random"]])
    _same(frs[0], ref(24000), "int16 streamed", summ[0])


def _zoo(n=64):
    """n clips of 0 .. 2 s with their own parameters and schedules, and what the rule says of each"""
    if "zoo" not in _cache:
        rng = np.random.default_rng(5)
        lens = [int(v) for v in rng.integers(0, 48001, n)]
        lens[:5] = [0, 1, 239, 48000, 880]
        prms = [V.Params(int(on), int(min(on, off)), int(mo), int(hg), int(hd), int(nm)) for on, off, mo, hg, hd, nm in
                zip(rng.integers(16, 4096, n), rng.integers(16, 200, n), rng.integers(1, 12, n), rng.integers(1, 60, n), rng.integers(0, 40, n),
                    rng.integers(1, 10 ** 8, n))]
        prms[3] = V.Params()
        clips = [talk(L, 100 + i, (110.0, 150.0, 220.0)[i % 3], 0.05 + 0.3 * (i % 4) / 3, spans=((0.1, 0.35), (0.5, 0.8))) for i, L in enumerate(lens)]
        scheds = [[int(rng.choice([0, 1, 7, 239, 240, 1920, 4000])) for _ in range(24)] for _ in range(n)]
        _cache["zoo"] = (clips, prms, scheds, [V.vad_ref(c, p) for c, p in zip(clips, prms)])
    return _cache["zoo"]


def test_64_streams_with_their_own_clips_parameters_and_chunks_in_one_call():
    _need_gpu()
    clips, prms, scheds, want = _zoo()
    assert sum(len(w.events) for w in want) > 40
    pool = _pool()
    frs, summ = _streamed(pool, list(range(64)), prms, clips, scheds)
    for i in range(64):
        _same(frs[i], want[i], ("all 64", i), summ[i])
    # a few of them again: other stream ids, reversed order, other company, other schedules
    pick, ids = [63, 40, 3, 17, 0], [5, 62, 9, 0, 33]
    frs, summ = _streamed(pool, ids, [prms[i] for i in pick], [clips[i] for i in pick], [scheds[(i + 7) % 64] for i in pick])
    for i, fr, sm in zip(pick, frs, summ):
        _same(fr, want[i], ("subset", i), sm)
    frs, summ = _streamed(pool, ids[::-1], [prms[i] for i in pick[::-1]], [clips[i] for i in pick[::-1]], [scheds[i] for i in pick[::-1]])
    for i, fr, sm in zip(pick[::-1], frs, summ):
        _same(fr, want[i], ("reversed", i), sm)


def test_detect_of_64_clips():
    _need_gpu()
    from sesameai.vad import detect
    clips, prms, _, want = _zoo()
    frs, summ = detect([_t(c) for c in clips], [_prm(p) for p in prms], want_summary=True)
    for i in range(64):
        _same(frs[i], want[i], ("detect", i), summ[i])
        assert frs[i].first == 0
    one = detect([_t(clips[3]).cuda()])
    _same(one[0], want[3], "detect alone, defaults")


def test_final_then_reuse_and_a_reset_in_the_middle_of_a_clip():
    _need_gpu()
    pool = _pool()
    a, b = clip(24000), clip(50011)
    pool.reset([2], _prm(QUICK))
    assert pool.poll()[2] == (False, 0, -1, -1, 0, 0, 0), "a reset stream reads as fresh whatever the device holds"
    first = pool.feed([2], [_t(a)], final=True)[0]
    _same(first, ref(24000), "first clip")
    again = [pool.feed([2], [_t(b[:30000])])[0], pool.feed([2], [_t(b[30000:])], final=True)[0]]      # final left the stream fresh, same parameters
    assert again[0].first == 0 and again[1].first == 125
    _same(_cat(again), ref(50011), "after final", pool.poll()[2])
    pool.feed([2], [_t(a[:10000])])                                    # an open clip: carry and state on the device
    pool.reset([2], _prm(V.Params()))
    fr = pool.feed([2], [_t(b)], final=True)[0]
    _same(fr, V.vad_ref(b), "after a reset", pool.poll()[2])


def test_the_decisive_inputs():
    _need_gpu()
    from sesameai.vad import detect
    two = talk(72000, 10, 150.0, 0.3, spans=((0.1, 0.3), (0.4, 0.6)))
    burst = noise(72000, 8, 0.001)
    burst[12000:19200] += noise(7200, 9, 0.3)
    for at in (30000, 36000, 36500, 50000):
        burst[at:at + 20] += 0.5
    bad = clip(24000)[:12000].copy(); bad[5000] = np.nan
    inf = bad.copy(); inf[5000] = -np.inf; inf[7000] = np.inf
    zero = bad.copy(); zero[5000] = 0.0
    mid = np.concatenate([np.zeros(4800, dtype=np.float32), voice(4800, 150.0, 0.3, 2, 0.0), voice(24000, 150.0, 0.00111, 1, 0.0)])
    cases = [("220 Hz first crossing", voice(12000, 220.0, 0.3, 1, 0.002), V.Params()), ("quiet pulses", pulses(24000), V.Params()),
             ("white noise", noise(48000, 7, 0.1), V.Params()), ("burst and clicks", burst, V.Params()), ("hang 70", two, V.Params(hang=70)),
             ("hang 20", two, V.Params(hang=20)), ("full-scale square", full_scale_square(), V.Params()),
             ("all -32768", np.full(4800, -4.0, dtype=np.float32), V.Params()), ("silence", np.zeros(4800, dtype=np.float32), V.Params()),
             ("nan", bad, QUICK), ("inf", inf, QUICK), ("between the thresholds", mid, V.Params())]
    frs, summ = detect([_t(x) for _, x, _ in cases], [_prm(p) for _, _, p in cases], want_summary=True)
    want = {name: V.vad_ref(x, p) for name, x, p in cases}
    for (name, _, _), fr, sm in zip(cases, frs, summ):
        _same(fr, want[name], name, sm)
    got = {name: fr for (name, _, _), fr in zip(cases, frs)}
    lag = got["220 Hz first crossing"].lag.cpu().numpy()[10:]
    assert (lag != V.vad_ref(cases[0][1], pick="argmax").lag[10:]).all(), "an arg-max lag would differ in every frame"
    assert int((got["quiet pulses"].flags.cpu().numpy()[2:] & 2).astype(bool).sum()) == 98 > int(np.count_nonzero(V.vad_ref(cases[1][1], shift=6).flags[2:] & 2))
    assert not (got["white noise"].flags.cpu().numpy() & 2).any() and summ[3].starts == 0
    assert (summ[4].starts, summ[4].ends, summ[5].starts, summ[5].ends) == (1, 1, 2, 2)
    assert not got["silence"].lag.any() and np.array_equal(got["nan"].flags.cpu().numpy(), V.vad_ref(zero, QUICK).flags)
    assert summ[11].in_speech and summ[11].starts == 1 and summ[11].ends == 0


def test_parameters_at_their_bounds():
    _need_gpu()
    from sesameai.vad import detect
    x = talk(48000, 3, 150.0, 0.3, spans=((0.1, 0.3), (0.5, 0.7)))
    sets = [V.Params(4095, 16, 1000, 10000, 10000, 2 ** 40), V.Params(16, 16, 1, 1, 0, 1), V.Params(4095, 4095, 1, 10000, 0, 1),
            V.Params(16, 16, 1000, 1, 10000, 2 ** 40), V.Params(200, 16, 1, 1, 0, 1)]
    frs, summ = detect([_t(x)] * len(sets), [_prm(p) for p in sets], want_summary=True)
    want = [V.vad_ref(x, p) for p in sets]
    for p, fr, sm, w in zip(sets, frs, summ, want):
        _same(fr, w, p, sm)
    assert want[0].events == [] and len(want[1].events) == len(want[4].events) == 4 and len(want[2].events) == 1,"the bounds change what is decided"


def test_every_refusal_leaves_the_pool_usable():
    _need_gpu()
    from sesameai import _abi
    from sesameai.vad import VadPool, detect
    with pytest.raises(_abi.CsmError):
        VadPool(0)
    with pytest.raises(_abi.CsmError):
        VadPool(65)
    pool = VadPool(4)
    x = _t(clip(24000))
    pool.reset([1], _prm(QUICK))
    first = pool.feed([1], [x[:10007]])[0]
    for ids, ps in (([0, 0], None), ([4], None), ([-1], None), ([], None), ([0, 1, 2, 3, 0], None), ([0], _prm(V.Params(on_q4=4096))),
                    ([0], _prm(V.Params(off_q4=15))), ([0], _prm(V.Params(min_on=0))), ([0], _prm(V.Params(hang=10001))), ([0], _prm(V.Params(hold=-1))),
                    ([0, 1], [_prm(V.Params()), _prm(V.Params(n_min=0))])):
        with pytest.raises(_abi.CsmError):
            pool.reset(ids, ps)
    for ids in ([1, 1], [4], [-1], [], [0, 1, 2, 3, 1]):
        with pytest.raises(_abi.CsmError):
            pool.feed(ids, [x[:10]] * len(ids))
    with pytest.raises(_abi.CsmError):
        pool.frame_count(4, 10)
    with pytest.raises(_abi.CsmError):
        pool.frame_count(0, -1)
    lib, h = _abi.lib, pool._h
    one, off, ln, fin, no = (C.c_int32 * 1)(1), (C.c_long * 1)(0), (C.c_long * 1)(10), (C.c_int32 * 1)(0), (C.c_long * 1)(0)
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    assert lib.mimi_vad_pool_feed(h, one, off, ln, fin, 1, None, 0, p, p, p, p, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, off, ln, fin, 1, p, 0, None, p, p, p, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, off, ln, fin, 1, p, 0, p, p, p, None, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, off, ln, fin, 1, p, 2, p, p, p, p, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, off, ln, fin, 1, p, 0, p, p, p + 4, p, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, (C.c_long * 1)(-1), ln, fin, 1, p, 0, p, p, p, p, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, off, (C.c_long * 1)(-1), fin, 1, p, 0, p, p, p, p, no, None) == -1
    assert lib.mimi_vad_pool_feed(h, one, off, (C.c_long * 1)(2 ** 30 + 1), fin, 1, p, 0, p, p, p, p, no, None) == -1
    assert b"2^30" in lib.mimi_vad_pool_last_error(h)
    assert lib.mimi_vad_pool_summary(h, None, None) == -1
    with pytest.raises(ValueError):
        detect([])
    with pytest.raises(ValueError):
        detect([x] * 65)
    # stream 1 went on as if nothing had happened: no refusal moved its state
    rest = pool.feed([1], [x[10007:]], final=True)[0]
    assert rest.first == first.flags.shape[0] == 41
    _same(_cat([first, rest]), ref(24000), "after the refusals", pool.poll()[1])
