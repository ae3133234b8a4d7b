"""Host logic around true-peak detection (no GPU), against recording fakes: ``Limit()``, ``SegmentFinish()`` and ``limiter=None`` make the
calls made before and import nothing new; a ``Limit(true_peak=True)`` among a reset's limits makes ONE mimi_lim_pool_reset_tp with the
flags in list order; ``paired`` and the live batch carry the flag to the slot's reset, and a request's chunks move by the latency L + T
from its first chunk to its last; ``SegmentFinish(loudness=, true_peak=True)`` makes one mimi_tp_measure per finish call, writes the true
peaks into the peak column of exactly the clips that ask, and synchronises nothing; ``tts_service --true-peak`` reaches ``SegmentFinish``."""
import ctypes as C
import sys

import pytest
import torch

import loudness_ref as LD
import test_limiter_host_logic as LH
from test_host_logic import _ScriptedSlots
from test_leveler_host_logic import LENS
from test_loudness_host_logic import _finish, _finisher

T = 8


class _ResetLib:
    def __init__(self):
        self.calls = []

    def mimi_lim_pool_reset(self, h, ids, c, l, rho, hr, n):
        self.calls.append(("reset", [list(a[:n]) for a in (ids, c, l, rho, hr)], n))
        return 0

    def mimi_lim_pool_reset_tp(self, h, ids, c, l, rho, hr, tp, n):
        self.calls.append(("reset_tp", [list(a[:n]) for a in (ids, c, l, rho, hr, tp)], n))
        return 0


def _pool():
    from sesameai.limiter import LimiterPool
    pool = object.__new__(LimiterPool)                                  # (no handle: __del__ finds none)
    pool._lib, pool._h, pool.n_streams = _ResetLib(), None, 8
    pool._check = lambda rc: None
    return pool


def test_the_default_limit_makes_the_reset_made_before_and_a_flag_makes_one_reset_tp():
    from sesameai.limiter import TRUE_PEAK_TAPS, Limit, paired
    from sesameai.loudness import Level
    assert Limit() == Limit(-1.0, 120, 100.0, 0, 2, False) and Limit().latency == 120 and Limit(true_peak=True).latency == 120 + T == 120 + TRUE_PEAK_TAPS
    assert Limit(true_peak=True).params() == Limit().params() == (29203, 120, 27, 0)
    pool = _pool()
    pool.reset([3, 1], Limit())
    pool.reset([0, 5], [Limit(-3.0, 24), Limit(drive_shift=1, true_peak=False)])
    assert [c[0] for c in pool._lib.calls] == ["reset", "reset"] and pool._lib.calls[0] == ("reset", [[3, 1], [29203] * 2, [120] * 2, [27] * 2, [0] * 2], 2)
    pool.reset([2, 7, 4], [Limit(), Limit(lookahead=1, true_peak=True), Limit(-3.0, true_peak=True)])
    assert len(pool._lib.calls) == 3 and pool._lib.calls[2][0] == "reset_tp" and pool._lib.calls[2][1][0] == [2, 7, 4] and pool._lib.calls[2][1][5] == [0, 1, 1]
    assert pool._lib.calls[2][1][2] == [120, 1, 120]
    pool.reset([6], Limit(true_peak=True))
    assert pool._lib.calls[3] == ("reset_tp", [[6], [29203], [120], [27], [0], [1]], 1)
    with pytest.raises(ValueError):
        pool.reset([6], Limit(lookahead=481, true_peak=True))
    lo, lm = paired(Level(-19.0), Limit(true_peak=True))
    assert lm == Limit(drive_shift=2, true_peak=True) and lm.latency == 128 and paired(Level(-19.0), Limit())[1].true_peak is False


class _FakeTpLimiter(LH._FakeLimiter):
    """delays each stream by its Limit's LATENCY, as the real pool delays a true-peak stream"""

    def feed(self, ids, chunks, final=False):
        real = [self._limit[int(i)] for i in ids]
        for i, lm in zip(ids, real):
            self._limit[int(i)] = lm._replace(lookahead=lm.latency)
        try:
            return super().feed(ids, chunks, final)
        finally:
            for i, lm in zip(ids, real):
                self._limit[int(i)] = lm


def test_the_live_batch_hands_the_flag_to_the_slots_reset_and_the_tail_is_L_plus_T(monkeypatch):
    from sesameai.limiter import Limit
    monkeypatch.setattr(LH, "_FakeLimiter", _FakeTpLimiter)
    limits = [Limit(true_peak=True), True, Limit(lookahead=480, true_peak=True), None, Limit(-3.0, 24, true_peak=True), Limit(lookahead=1, true_peak=True),
              None, Limit(true_peak=False), True, Limit(drive_shift=1, true_peak=True), None]
    assert len(limits) == len(LENS)
    want = LH._want(limits)
    plain, pool0, _ = LH._run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3)
    got, pool1, made = LH._run(_ScriptedSlots, LENS, 30, monkeypatch, limiter=limits, first_chunk_frames=3)
    assert pool1.log == pool0.log and len(made["limit"]) == 1
    given = [l for call in made["limit"][0].resets for _, l in call]
    for i, l in enumerate(want):
        if l is not None and min(LENS[i], 30) > 0:
            given.remove(l)                                              # (ValueError: a request did not get ITS Limit, flag included)
    assert len(given) <= 1
    tails = 0
    for i, l in enumerate(want):
        a, b = [c for c in plain if c[0] == i], [c for c in got if c[0] == i]
        if l is None:
            assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
            continue
        la, lb, D = [x[1].shape[0] for x in a], [y[1].shape[0] for y in b], int(l.lookahead) + (T if l.true_peak else 0)
        taken = given_ = 0
        for j in range(len(la)):
            taken += la[j]
            ready = taken if j == len(la) - 1 else max(0, taken - D)
            assert lb[j] == ready - given_, (i, j, la, lb)
            given_ = ready
        assert lb[-1] == la[-1] + min(D, sum(la[:-1])) and sum(lb) == sum(la), (i, la, lb)
        tails += l.true_peak and len(la) > 1 and lb[-1] - la[-1] == D
    assert tails >= 3, "a request's last chunk carries L + T samples of tail"


def test_limiter_none_imports_nothing_new(monkeypatch):
    for name in ("sesameai.limiter", "sesameai.truepeak"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    import sesameai
    for name in ("limiter", "truepeak"):
        if hasattr(sesameai, name):
            monkeypatch.setattr(sesameai, name, getattr(sesameai, name))
    plain, pool0, _ = LH._run(_ScriptedSlots, LENS, 30, monkeypatch)
    got, pool1, made = LH._run(_ScriptedSlots, LENS, 30, monkeypatch, limiter=None)
    assert "sesameai.limiter" not in sys.modules and "sesameai.truepeak" not in sys.modules and pool1.log == pool0.log
    assert all(x[0] == y[0] and torch.equal(x[1], y[1]) for x, y in zip(plain, got))
    from sesameai.limiter import Limit  # noqa: F401  (a Limit alone does not bring the meter in)
    assert "sesameai.truepeak" not in sys.modules


class _TpLib:
    """records mimi_tp_measure; the rows it 'writes' are 1000 + clip index in the true-peak column"""

    def __init__(self):
        self.calls, self.bufs, self.packed = [], [], []                 # (packed: the buffer the loudness meter was handed, or None)

    def mimi_tp_measure(self, buf, offs, lens, n, fmt, out, stream):
        self.calls.append((n, list(offs[:n]), list(lens[:n]), fmt))
        self.bufs.append(buf)
        rows = (C.c_int64 * (4 * n)).from_address(out)
        for k in range(n):
            rows[4 * k:4 * k + 4] = [500 + k, 1000 + k, 0, lens[k]]
        return 0

    def mimi_tp_last_error(self):
        return b""


def _tp_finisher(monkeypatch):
    fin, lib, metered = _finisher(monkeypatch)
    from sesameai import _abi
    from sesameai import loudness as ld_mod
    tp = _TpLib()
    monkeypatch.setattr(_abi, "lib", tp)
    def measure_rows(wavs, device=None, packed=None):
        metered.append([int(w.shape[0]) for w in wavs])
        tp.packed.append(None if packed is None else packed.packed.data_ptr())
        return torch.arange(4 * len(wavs), dtype=torch.int64).reshape(len(wavs), 4)
    monkeypatch.setattr(ld_mod, "measure_rows", measure_rows)
    syncs = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    for name in ("cpu", "item", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **k: (syncs.append(_name), _real(self, *a, **k))[1])
    return fin, lib, metered, tp, syncs


def test_segment_finish_defaults_make_the_calls_made_before(monkeypatch):
    fin, lib, metered, tp, syncs = _tp_finisher(monkeypatch)
    clips = [torch.zeros(n) for n in (10, 0, 25)]
    assert _finish() == _finish(true_peak=False) and _finish().true_peak is False
    fin.finish(clips, _finish(0, 0, 0))
    fin.finish(clips, _finish(0, 0, 0, true_peak=True))                 # without a loudness the flag asks for nothing
    assert [c[0] for c in lib.calls] == ["plain", "plain"] and metered == [] and tp.calls == []
    fin.finish(clips, _finish(0, 0, 0, loudness=-19.0))
    assert lib.calls[2][0] == "ld" and metered == [[10, 0, 25]] and tp.calls == [] and tp.packed == [None]      # the meter packs for itself, as before
    assert fin.last_meter.tolist() == torch.arange(12).reshape(3, 4).tolist()          # the meter's own peaks, untouched


def test_true_peak_makes_one_measure_per_finish_call_and_writes_the_peak_column_without_a_synchronisation(monkeypatch):
    fin, lib, metered, tp, syncs = _tp_finisher(monkeypatch)
    clips = [torch.zeros(n) for n in (10, 0, 25, 7)]
    how = [_finish(0, 0, 0, loudness=-19.0, true_peak=True), _finish(0, 0, 0), _finish(0, 0, 0, loudness=-23.0, ceiling_db=-3.0),
           _finish(0, 0, 0, loudness=-16.0, ceiling_db=-2.0, true_peak=True)]
    out = fin.finish(clips, how)
    assert syncs == [], syncs
    assert metered == [[10, 0, 25, 7]] and tp.calls == [(4, [0, 10, 10, 35], [10, 0, 25, 7], 0)] and len(lib.calls) == 1
    assert tp.bufs == tp.packed and tp.bufs[0] is not None, "both meters read ONE packed buffer: the clips are not packed a second time"
    kind, m, n_in, pt, ceiling, meter = lib.calls[0]
    assert (kind, m, n_in) == ("ld", 4, [10, 0, 25, 7]) and meter == fin.last_meter.data_ptr()
    assert pt == [LD.target_ms(-19.0), 0, LD.target_ms(-23.0), LD.target_ms(-16.0)] and ceiling == [LD.ceiling_i16(-1.0), 32767, LD.ceiling_i16(-3.0), LD.ceiling_i16(-2.0)]
    rows = fin.last_meter.tolist()                                       # S, n and hops stay; the peak column of clips 0 and 3 is the true peak
    assert rows == [[0, 1, 1000, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 1003, 15]] and [int(o.shape[0]) for o in out] == [10, 0, 25, 7]
    # 70 clips are two finish calls: one measure each, only where a clip of the call asks
    lib.calls.clear(); metered.clear(); tp.calls.clear()
    fin.finish([torch.zeros(5)] * 70, [_finish(0, 0, 0, loudness=-19.0, true_peak=True)] * 64 + [_finish(0, 0, 0, loudness=-19.0)] * 6)
    assert [c[:2] for c in lib.calls] == [("ld", 64), ("ld", 6)] and [c[0] for c in tp.calls] == [64] and len(metered) == 2


def test_the_service_reads_true_peak_with_loudness(tmp_path, capsys):
    from test_say_batch_host_logic import TEXT, Gen, _module, _tts
    mod = _module()
    args = mod.parse_args(["hello", "--batch", "2", "--loudness", "-19", "--true-peak"])
    assert args.true_peak is True and mod.parse_args(["hello"]).true_peak is False
    with pytest.raises(SystemExit):
        mod.parse_args(["hello", "--batch", "2", "--true-peak"])
    capsys.readouterr()
    assert mod.TTS(voice_dir="/nonexistent", loudness=-19, true_peak=True).true_peak is True and mod.TTS(voice_dir="/nonexistent").true_peak is False
    gen = Gen()
    tts = _tts(gen)
    tts.say(TEXT, output_filename=None, batch=3, loudness=-19)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-19.0, ceiling_db=-1.0) and gen.segment_calls[-1]["finish"].true_peak is False
    tts.say(TEXT, output_filename=None, batch=3, loudness=-19, true_peak=True)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-19.0, ceiling_db=-1.0, true_peak=True)
    for call in (lambda: tts.say(TEXT, output_filename=None, true_peak=True), lambda: tts.export_wav(TEXT, str(tmp_path / "b.wav"), true_peak=True)):
        with pytest.raises(ValueError, match="true_peak= needs batch="):     # as loudness= without batch=
            call()
    tts.say(TEXT, output_filename=None, batch=3, true_peak=True)             # without a loudness the flag is not read
    assert gen.segment_calls[-1]["finish"] == _finish()
    tts.export_wav(TEXT, str(tmp_path / "a.wav"), batch=2, loudness=-23.0, true_peak=True)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-23.0, true_peak=True)
    tts.loudness, tts.true_peak = -16.0, True                               # the service's own, and a call's own over it
    tts.say(TEXT, output_filename=None, batch=3)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-16.0, true_peak=True)
    tts.say(TEXT, output_filename=None, batch=3, true_peak=False)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-16.0)
