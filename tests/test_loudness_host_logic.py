"""Host logic around the loudness pool (no GPU): ``loudness=`` of ``TTS`` / ``say`` / ``export_wav`` / ``--loudness`` on the scripted generator
of tests/test_say_batch_host_logic.py, ``SegmentFinisher.finish`` against a recording fake of the library -- ``loudness=None`` makes the
call made before and nothing else; a target on any clip meters the call's clips once and makes the ONE levelling call with per-clip
integers -- and the LUFS -> integer conversions against tests/loudness_ref.py."""
import contextlib
import types

import pytest
import torch

import loudness_ref as L
from test_say_batch_host_logic import Gen, TEXT, _module, _tts


def _finish(*a, **kw):
    from sesameai.finish import SegmentFinish
    return SegmentFinish(*a, **kw)


def test_say_batch_hands_the_target_to_the_finisher(tmp_path):
    gen = Gen()
    tts = _tts(gen)
    tts.say(TEXT, output_filename=None, batch=3, loudness=-19)
    assert gen.segment_calls[-1]["finish"] == _finish(lead_ms=500, tail_ms=100, fade_ms=50, loudness=-19.0, ceiling_db=-1.0)
    tts.say(TEXT, output_filename=None, batch=3)
    assert gen.segment_calls[-1]["finish"] == _finish(lead_ms=500, tail_ms=100, fade_ms=50) and gen.segment_calls[-1]["finish"].loudness is None
    tts.export_wav(TEXT, str(tmp_path / "a.wav"), batch=2, loudness=-23.5)
    assert gen.segment_calls[-1]["finish"].loudness == -23.5
    # the service's own target, and a call's own over it
    tts.loudness, tts.ceiling_db = -16.0, -3.0
    tts.say(TEXT, output_filename=None, batch=3)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-16.0, ceiling_db=-3.0)
    tts.say(TEXT, output_filename=None, batch=3, loudness=-30)
    assert gen.segment_calls[-1]["finish"] == _finish(loudness=-30.0, ceiling_db=-3.0)
    assert gen.codes_calls == 0


def test_loudness_needs_batch(tmp_path):
    tts = _tts(Gen())
    with pytest.raises(ValueError, match="loudness= needs batch="):
        tts.say(TEXT, output_filename=None, loudness=-19)
    with pytest.raises(ValueError, match="loudness= needs batch="):
        tts.export_wav(TEXT, str(tmp_path / "a.wav"), loudness=-19)
    tts.loudness = -19.0
    with pytest.raises(ValueError, match="loudness= needs batch="):
        tts.say(TEXT, output_filename=None)


def test_the_command_line(capsys):
    mod = _module()
    args = mod.parse_args(["--batch", "4", "--loudness", "-19", "hello"])
    assert args.loudness == -19.0 and args.batch == 4
    assert mod.parse_args(["hello"]).loudness is None
    for bad in (["--loudness", "-19", "hello"], ["--batch", "4", "--loudness", "3", "hello"], ["--batch", "4", "--loudness", "-71", "hello"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    capsys.readouterr()
    assert mod.TTS(voice_dir="/nonexistent", loudness=-19).loudness == -19 and mod.TTS(voice_dir="/nonexistent").loudness is None


def test_the_conversions_are_the_references():
    from sesameai import loudness as ld
    for v in (-70, -30.5, -23, -19, -16, -14, -0.691, 0):
        assert ld.target_ms(v) == L.target_ms(v) > 0
    assert ld.target_ms(-0.691) == 2 ** 30 and ld.target_ms(0) < 2 ** 31
    for v in (0, -0.1, -1, -3, -6.02, -20, -120):
        assert ld.ceiling_i16(v) == L.ceiling_i16(v)
    assert ld.ceiling_i16(0) == 32767 and ld.ceiling_i16(-1) == 29203 and ld.ceiling_i16(-120) == 1
    for bad in (0.5, -70.5, float("nan")):
        with pytest.raises(ValueError):
            ld.target_ms(bad)
    with pytest.raises(ValueError):
        ld.ceiling_i16(0.1)
    assert ld.lufs(0, 0) == float("-inf") and abs(ld.lufs(2 ** 30 * 4 * ld.HOP, 1) + 0.691) < 1e-12 and ld.lufs(12345, 7) == L.lufs(12345, 7)
    assert ld.Loudness(2 ** 30 * 4 * ld.HOP * 3, 3, 100, 9).lufs == ld.lufs(2 ** 30 * 4 * ld.HOP, 1)
    assert (ld.HOP, ld.ROW, ld.MAX_STREAMS) == (L.H, 4, 64)
    assert _finish().level() == (0, 32767) and _finish(loudness=-19).level() == (L.target_ms(-19), L.ceiling_i16(-1.0))
    assert _finish(loudness=-19, ceiling_db=-6).level() == (L.target_ms(-19), L.ceiling_i16(-6))


def test_one_target_or_one_per_request():
    from sesameai.loudness import per_request
    assert per_request(None, 3) == [None] * 3 and per_request(-19, 2) == [-19.0, -19.0]
    assert per_request([-19, None, -23.5], 3) == [-19.0, None, -23.5]
    with pytest.raises(ValueError):
        per_request([-19, -20], 3)


class _Lib:
    """records the finisher's calls; writes the offsets a real call would"""

    def __init__(self):
        self.calls = []

    def mimi_fin_create(self, out):
        return 0

    def mimi_fin_destroy(self, h):
        pass

    def mimi_fin_out_count(self, n, lead, tail):
        return n + lead + tail

    def _lay_out(self, n_in, lead, tail, m, off, n_out):
        o = 0
        for k in range(m):
            off[k], n_out[k] = o, n_in[k] + lead[k] + tail[k]
            o += n_out[k]

    def mimi_fin_segments(self, h, ptrs, n_in, lead, tail, fade, m, out, off, n_out, stream):
        self.calls.append(("plain", m, list(n_in[:m])))
        self._lay_out(n_in, lead, tail, m, off, n_out)
        return 0

    def mimi_fin_segments_ld(self, h, ptrs, n_in, lead, tail, fade, pt, ceiling, meter, m, out, off, n_out, stream):
        self.calls.append(("ld", m, list(n_in[:m]), list(pt[:m]), list(ceiling[:m]), meter))
        self._lay_out(n_in, lead, tail, m, off, n_out)
        return 0


def _finisher(monkeypatch):
    from sesameai import finish as fin_mod
    from sesameai import loudness as ld_mod
    lib, metered = _Lib(), []
    monkeypatch.setattr(fin_mod, "lib", lib)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))

    def measure_rows(wavs, device=None):
        metered.append([int(w.shape[0]) for w in wavs])
        return torch.zeros((len(wavs), 4), dtype=torch.int64)
    monkeypatch.setattr(ld_mod, "measure_rows", measure_rows)
    return fin_mod.SegmentFinisher("cpu"), lib, metered


def test_no_target_makes_the_call_made_before_and_nothing_else(monkeypatch):
    fin, lib, metered = _finisher(monkeypatch)
    clips = [torch.zeros(n) for n in (10, 0, 25)]
    out = fin.finish(clips, _finish(lead_ms=1, tail_ms=0, fade_ms=0))
    assert lib.calls == [("plain", 3, [10, 0, 25])] and metered == [] and fin.last_meter is None
    assert [int(o.shape[0]) for o in out] == [34, 24, 49]
    fin.finish(clips, [_finish(), _finish(loudness=None, ceiling_db=-6.0), _finish()])          # a ceiling alone asks for nothing
    assert [c[0] for c in lib.calls] == ["plain", "plain"] and metered == []


def test_a_target_on_any_clip_meters_the_call_once_and_levels_per_clip(monkeypatch):
    fin, lib, metered = _finisher(monkeypatch)
    clips = [torch.zeros(n) for n in (10, 0, 25)]
    out = fin.finish(clips, [_finish(lead_ms=0, tail_ms=0, fade_ms=0), _finish(0, 0, 0, loudness=-19.0), _finish(0, 0, 0, loudness=-23.0, ceiling_db=-3.0)])
    assert metered == [[10, 0, 25]] and len(lib.calls) == 1
    kind, m, n_in, pt, ceiling, meter = lib.calls[0]
    assert (kind, m, n_in) == ("ld", 3, [10, 0, 25])
    assert pt == [0, L.target_ms(-19.0), L.target_ms(-23.0)] and ceiling == [32767, L.ceiling_i16(-1.0), L.ceiling_i16(-3.0)]
    assert meter == fin.last_meter.data_ptr() and [int(o.shape[0]) for o in out] == [10, 0, 25]
    # 70 clips are two calls; only the one that holds a target is metered
    lib.calls.clear(); metered.clear()
    fin.finish([torch.zeros(5)] * 70, [_finish(0, 0, 0)] * 64 + [_finish(0, 0, 0, loudness=-19.0)] * 6)
    assert [c[:2] for c in lib.calls] == [("plain", 64), ("ld", 6)] and metered == [[5] * 6]
