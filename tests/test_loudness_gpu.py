"""The device loudness pool and the levelling finisher (include/mimi_hip.h mimi_ld_pool_* and mimi_fin_segments_ld, sesameai/loudness.py,
sesameai/finish.py) against the rule (tests/loudness_ref.py): every comparison is np.array_equal -- hop energies, {S, n, peak, hops} and
finished samples; one-shot and streamed over the oracle test's schedules, fp32 and int16, in any company, order and stream id, after
final, on a ring that wraps, and through the finisher with and without a target."""
import numpy as np
import pytest
import torch

import finish_ref
import loudness_ref as L
from test_loudness_oracle import SCHEDULES, clip, cuts, speechlike

pytestmark = pytest.mark.gpu
_cache = {}
LENGTHS = [0, 1, L.T - 2, L.T - 1, 2399, 2400, 2401, 9599, 9600, 9601, 24007]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pool(n=64, ring=0):
    from sesameai.loudness import LoudnessPool
    if ("pool", n, ring) not in _cache:
        _cache[("pool", n, ring)] = LoudnessPool(n, ring=ring)
    return _cache[("pool", n, ring)]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _source():
    """speech, then the full-scale square: every length cut from it holds both"""
    if "src" not in _cache:
        _cache["src"] = np.concatenate([clip("speech 0.9")[3000:15000], clip("square 3 kHz")[:9000], clip("speech 0.05")[:6000]])
    return _cache["src"]


def _ref(x, ring=L.RING):
    """(hop energies, (S, n, peak, hops)) of one clip, kept"""
    key = ("ref", x.dtype.str, x.shape[0], hash(x.tobytes()), ring)
    if key not in _cache:
        _cache[key] = (L.hop_energies(L.to_s(x)), L.measure_ref(x, ring))
    return _cache[key]


def _one_shot(pool, clips):
    ids = list(range(len(clips)))
    pool.reset(ids)
    assert [pool.hop_count(i, c.shape[0], True) for i, c in zip(ids, clips)] == [c.shape[0] // L.H for c in clips]
    e = pool.feed(ids, [_t(c) for c in clips], final=True)
    rows = pool.integrate(ids).cpu().tolist()
    return [v.cpu().numpy() for v in e], [tuple(r) for r in rows]


def test_clips_of_every_length_and_kind_are_the_rule():
    _need_gpu()
    src = _source()
    bad = np.array([np.nan, np.inf, -np.inf, 0.5] * 3000, np.float32)
    clips = [src[:N] for N in LENGTHS] + [src[7:7 + N][::-1].copy() for N in LENGTHS]
    clips += [bad, np.zeros(12000, np.float32), (speechlike(1.0, 1.0, 5) * np.float32(10 ** (-75 / 20))), clip("square 3 kHz")[:12001],
              np.full(4801, -1.0, np.float32), clip("plosive")[24000:40000]]
    for kind, cs in (("fp32", clips), ("int16", [L.to_s(c).astype(np.int16) for c in clips])):
        got_e, got_rows = _one_shot(_pool(), cs)
        for j, c in enumerate(cs):
            want_e, want = _ref(c)
            assert got_e[j].dtype == np.int64 and np.array_equal(got_e[j], want_e), (kind, j, c.shape[0])
            assert got_rows[j] == want, (kind, j, c.shape[0], got_rows[j], want)
    assert _ref(bad)[1][2] == 16384 and _ref(clips[-5])[1][:2] == (0, 0) and _ref(clips[-4])[1][:2] == (0, 0)
    assert _ref(clips[-3])[1][1] > 0 and _ref(clips[-2])[1][2] == 32768


def _streamed(pool, ids, clips, steps):
    """Every clip through its own stream on its own schedule, all streams sharing the calls; then an empty chunk with final.
    -> per stream its hop energies, concatenated, and its row after its final call."""
    pool.reset(ids)
    dev = [_t(c).cuda() for c in clips]
    plans = [cuts(c.shape[0], s) for c, s in zip(clips, steps)]
    out, rows = [[] for _ in ids], [None] * len(ids)
    for t in range(max(len(p) for p in plans) + 1):
        live = [j for j in range(len(ids)) if t <= len(plans[j])]
        fin = [t == len(plans[j]) for j in live]
        chunks = [dev[j][:0] if f else dev[j][plans[j][t][0]:plans[j][t][1]] for j, f in zip(live, fin)]
        counts = [pool.hop_count(ids[j], c.shape[0], f) for j, c, f in zip(live, chunks, fin)]
        es = pool.feed([ids[j] for j in live], chunks, fin)
        assert [int(e.shape[0]) for e in es] == counts
        got = pool.integrate([ids[j] for j in live]).cpu().tolist() if any(fin) else None
        for a, (j, e, f) in enumerate(zip(live, es, fin)):
            out[j].append(e)
            if f:
                rows[j] = tuple(got[a])
    return [torch.cat(v).cpu().numpy() for v in out], rows


def test_one_stream_over_the_schedules_is_the_one_shot_result():
    _need_gpu()
    src, pool = _source(), _pool()
    jobs = [(N, name) for N in (2401, 9601, 24007) for name in SCHEDULES if N == 2401 or name != "7"]      # (7 by 7: 343 calls)
    ids = list(range(len(jobs)))
    got_e, got_rows = _streamed(pool, ids, [src[:N] for N, _ in jobs], [SCHEDULES[name] for _, name in jobs])
    for j, (N, name) in enumerate(jobs):
        want_e, want = _ref(src[:N])
        assert np.array_equal(got_e[j], want_e) and got_rows[j] == want, (N, name)
    # alone in its calls, on another id, sample by sample across the hop edges
    e, rows = _streamed(pool, [37], [src[:9601]], [1])
    assert np.array_equal(e[0], _ref(src[:9601])[0]) and rows[0] == _ref(src[:9601])[1]


def test_64_ragged_streams_in_any_order_and_after_final():
    _need_gpu()
    src, pool = _source(), _pool()
    rng = np.random.default_rng(11)
    lens = [int(v) for v in rng.integers(0, 24008, 64)]
    lens[:4] = [24007, 0, 2400, 9599]
    starts = [int(v) for v in rng.integers(0, src.shape[0] - 24007, 64)]
    clips = [src[a:a + n] for a, n in zip(starts, lens)]
    steps = [list(SCHEDULES.values())[1:][j % 6] if j % 7 else None for j in range(64)]
    steps = [s if s != 1 else 2399 for s in steps]
    ids = [int(v) for v in rng.permutation(64)]
    got_e, got_rows = _streamed(pool, ids, clips, steps)
    for j, c in enumerate(clips):
        assert np.array_equal(got_e[j], _ref(c)[0]) and got_rows[j] == _ref(c)[1], (j, c.shape[0], steps[j])
    # the same streams, the list reversed, with no reset between: `final` left every one of them fresh
    pool2_e = pool.feed(ids[::-1], [_t(c) for c in clips[::-1]], final=True)
    rows = [tuple(r) for r in pool.integrate(ids[::-1]).cpu().tolist()]
    for j, c in enumerate(clips[::-1]):
        assert np.array_equal(pool2_e[j].cpu().numpy(), _ref(c)[0]) and rows[j] == _ref(c)[1], (j, c.shape[0])
    # a stream that was reset and not fed reads as zeros; one that was cut short by a reset starts afresh
    pool.feed([3], [_t(src[:5000])])
    pool.reset([3, 4])
    assert [tuple(r) for r in pool.integrate([3, 4]).cpu().tolist()] == [(0, 0, 0, 0)] * 2
    e = pool.feed([3], [_t(src[:9601])], final=True)
    assert np.array_equal(e[0].cpu().numpy(), _ref(src[:9601])[0]) and tuple(pool.integrate([3]).cpu().tolist()[0]) == _ref(src[:9601])[1]


def test_a_ring_that_wraps_integrates_the_hops_it_holds():
    _need_gpu()
    pool = _pool(2, ring=8)
    x = clip("loud then quiet")[60000:120000]                 # 25 hops across the drop of 38 dB
    st = L.StreamRef(ring=8)
    for a, b in ((0, 31000), (31000, 40000), (40000, 60000)):
        e = pool.feed([1], [_t(x[a:b])])
        assert np.array_equal(e[0].cpu().numpy(), st.feed(x[a:b]))
        assert tuple(pool.integrate([1]).cpu().tolist()[0]) == st.integrate(), (a, b)
    S, n = L.gate(L.hop_energies(L.to_s(x))[-8:], 8)
    assert st.integrate()[:2] == (S, n) and (S, n) != L.gate(L.hop_energies(L.to_s(x)))
    # one call of more hops than the ring holds
    pool.reset([0])
    pool.feed([0], [_t(x)], final=True)
    assert tuple(pool.integrate([0]).cpu().tolist()[0]) == (S, n, int(np.abs(L.to_s(x)).max()), 25)


def test_the_library_refuses_what_the_header_says():
    _need_gpu()
    from sesameai._abi import CsmError
    from sesameai.loudness import LoudnessPool
    for n, ring in ((0, 0), (65, 0), (4, 3), (4, 4097)):
        with pytest.raises(CsmError):
            LoudnessPool(n, ring=ring)
    pool = _pool()
    pool.reset([0, 1])
    pool.feed([0], [_t(_source()[:100])])
    for ids in ([], [0, 0], [64], [-1]):
        with pytest.raises(CsmError):
            pool.feed(ids, [_t(_source()[:10])] * len(ids))
        with pytest.raises(CsmError):
            pool.integrate(ids)
    e = pool.feed([0], [_t(_source()[100:2401])], final=True)        # nothing moved: the hop completes as if no call had been refused
    assert np.array_equal(e[0].cpu().numpy(), _ref(_source()[:2401])[0])


def _fin():
    from sesameai.finish import SegmentFinisher
    if "fin" not in _cache:
        _cache["fin"] = SegmentFinisher()
    return _cache["fin"]


def test_64_ragged_clips_with_and_without_a_target_are_the_rule():
    _need_gpu()
    from sesameai.finish import SegmentFinish
    from sesameai.loudness import lufs, measure
    src = _source()
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(0, 30000, 64)]
    lens[:8] = [0, 1, 9599, 9600, 27000, 16000, 12000, 12345]
    clips = [src[:n].copy() for n in lens]
    clips[5] = clip("plosive")[24000:40000]                   # the ceiling binds
    clips[6] = np.zeros(12000, np.float32)                    # nothing above the gate: the peak rule
    clips[7][100] = np.nan
    fins = []
    for j in range(64):
        target = None if j % 3 == 2 else (-19.0, -23.0, -30.0, -16.0)[j % 4]
        fins.append(SegmentFinish(lead_ms=(0, 500, 7)[j % 3] if j > 8 else 0, tail_ms=(100, 0)[j % 2] if j > 8 else 0,
                                  fade_ms=(50, 0, 3)[j % 3] if j > 8 else 0, loudness=target, ceiling_db=(-1.0, -3.0)[j % 2]))
    fins[4] = SegmentFinish(0, 0, 0, loudness=-19.0)
    fins[5] = SegmentFinish(0, 0, 0, loudness=-19.0)
    got = [y.cpu().numpy() for y in _fin().finish([_t(c) for c in clips], fins)]
    plain = [y.cpu().numpy() for y in _fin().finish([_t(c) for c in clips], [SegmentFinish(f.lead_ms, f.tail_ms, f.fade_ms) for f in fins])]
    bound_seen = set()
    for j, (c, f) in enumerate(zip(clips, fins)):
        lead, tail, fade = f.samples(24000)
        P_T, C = f.level()
        assert (P_T, C) == ((L.target_ms(f.loudness), L.ceiling_i16(f.ceiling_db)) if f.loudness is not None else (0, 32767))
        want = L.finish_ld_ref(c, lead, tail, fade, P_T, C)
        assert got[j].dtype == np.int16 and np.array_equal(got[j], want), (j, c.shape[0], f, int(np.count_nonzero(got[j] != want)))
        assert np.array_equal(plain[j], finish_ref.finish_ref(c, lead, tail, fade)), j
        if f.loudness is None or L.measure_ref(c)[1] == 0:
            assert np.array_equal(got[j], plain[j]), j        # bit for bit mimi_fin_segments' output
        else:
            S, n, peak, _ = L.measure_ref(c)
            bound_seen.add(L.clip_gain(S, n, peak, P_T, C)[1])
    assert bound_seen == {True, False}
    assert L.clip_gain(*L.measure_ref(clips[5])[:3], *fins[5].level())[1] and not L.clip_gain(*L.measure_ref(clips[4])[:3], *fins[4].level())[1]
    # the finished clip reads its target on the meter where the ceiling did not bind (from the integer results)
    after = measure([_t(got[4]), _t(got[5])])
    assert (after[0].S, after[0].n, after[0].peak, after[0].hops) == L.measure_ref(got[4])
    assert abs(lufs(after[0].S, after[0].n) + 19.0) <= 0.1
    assert after[1].lufs < -19.0 and abs(after[1].peak - L.ceiling_i16(-1.0)) <= 2


def test_more_than_64_clips_and_no_target_makes_the_old_call():
    _need_gpu()
    from sesameai.finish import SegmentFinish
    src = _source()
    clips = [src[100 * j:100 * j + 9600 + 37 * j] for j in range(70)]
    fins = [SegmentFinish(10, 5, 2, loudness=-20.0 if j % 2 else None) for j in range(70)]
    got = _fin().finish([_t(c) for c in clips], fins)
    for j in (0, 1, 63, 64, 65, 69):
        lead, tail, fade = fins[j].samples(24000)
        assert np.array_equal(got[j].cpu().numpy(), L.finish_ld_ref(clips[j], lead, tail, fade, *fins[j].level())), j
    fin = _fin()
    fin.last_meter = None
    fin.finish([_t(clips[0])], SegmentFinish(10, 5, 2))
    assert fin.last_meter is None
