"""Host logic around the time-stretch pool (no GPU): SlotStreams (sesameai/live_batch.py, through Generator.generate_many_stream) against
recording fake pools, Generator.generate_segments' one stretch call per block, and ``speed=`` / ``--speed`` of the TTS service.  The fake
stretcher is a pure delay -- it holds a stream's last LOOK samples back until ``final`` -- so a request's samples come out once, in order,
exactly when the tail is carried; what is checked is the bookkeeping: today's calls when no speed is given, ONE stretch call per decode
call in front of the resampler's, ``final`` on closing chunks, a tail for a closing chunk that is empty, and resets that carry the speed."""
import pytest
import torch

from test_first_chunk_host_logic import _Codec
from test_host_logic import _ScriptedSlots, _ScriptedSlotsBeside
from test_resample_host_logic import _FakeResampler
from test_say_batch_host_logic import Gen, TEXT, _module, _tts
from test_streams_host_logic import _scripts

LOOK = 7
EVENTS = []                          # ("stretch" | "resample", the call) in the order the fakes were called


class _FakeStretcher:
    def __init__(self, n=3, device="cpu"):
        self.n_streams, self.calls, self.resets = n, [], []
        self._held = [torch.empty(0) for _ in range(n)]

    def reset(self, ids, speeds):
        ids, speeds = [int(i) for i in ids], [float(s) for s in speeds]
        assert len(ids) == len(speeds) >= 1
        self.resets.append(list(zip(ids, speeds)))
        for i in ids:
            self._held[i] = torch.empty(0)

    def feed(self, ids, chunks, final=False, want_offsets=False):
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, bool) else [bool(f) for f in final]
        assert len(set(ids)) == len(ids) == len(chunks) == len(fin) >= 1 and all(0 <= i < self.n_streams for i in ids)
        self.calls.append([(i, int(c.shape[0]), f) for i, c, f in zip(ids, chunks, fin)])
        EVENTS.append(("stretch", self.calls[-1]))
        out = []
        for i, c, f in zip(ids, chunks, fin):
            assert c.dim() == 1 and c.dtype == torch.float32
            x = torch.cat([self._held[i], c.cpu()])
            keep = 0 if f else min(LOOK, x.shape[0])
            out.append(x[:x.shape[0] - keep])
            self._held[i] = x[x.shape[0] - keep:]
        return out


class _LoggedResampler(_FakeResampler):
    def feed(self, ids, chunks, final=False):
        out = super().feed(ids, chunks, final)
        EVENTS.append(("resample", self.calls[-1]))
        return out


def _run(model_cls, lens, limit, monkeypatch, **kw):
    from sesameai import resample as rs_mod
    from sesameai import stretch as ts_mod
    from sesameai.generator import Generator
    made, made_rs = [], []
    monkeypatch.setattr(ts_mod, "TimeStretchPool", lambda *a, **k: made.append(_FakeStretcher(*a, **k)) or made[-1])
    monkeypatch.setattr(rs_mod, "ResamplerPool", lambda *a, **k: made_rs.append(_LoggedResampler(*a, **k)) or made_rs[-1])
    del EVENTS[:]
    codec = _Codec([])
    gen = Generator(model_cls(_scripts(lens, 11), 3), audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    texts = list(range(len(lens)))
    chunks = list(gen.generate_many_stream(texts, [0] * len(lens), [[]] * len(lens), max_audio_length_ms=limit * 80, **kw))
    return chunks, codec.pools[0], made, made_rs


LENS = [3, 17, 0, 5, 40, 11, 20, 1, 22, 10, 33]
SPEEDS = [1.2, None, 0.8, 1.2, 2.0, None, 0.5, 1.0, 1.2, 1.5, 0.73]           # (1.0 is None: no call at all)


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_no_speed_builds_no_stretcher_and_makes_todays_calls(model_cls, monkeypatch):
    plain, pool0, made0, _ = _run(model_cls, LENS, 30, monkeypatch)
    for speed in (None, 1.0, [None] * len(LENS), [1.0, None] * 5 + [1]):
        got, pool1, made, _ = _run(model_cls, LENS, 30, monkeypatch, speed=speed)
        assert made == [] and EVENTS == [], "no speed: no stretcher is built"
        assert pool1.log == pool0.log and len(got) == len(plain)
        assert all(a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(plain, got))


@pytest.mark.parametrize("first", [None, 3])
@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_slot_streams_stretch_every_decode_call_once_and_close_with_the_tail(model_cls, first, monkeypatch):
    kw = {} if first is None else {"first_chunk_frames": first}
    plain, pool0, _, _ = _run(model_cls, LENS, 30, monkeypatch, **kw)
    got, pool1, made, _ = _run(model_cls, LENS, 30, monkeypatch, speed=SPEEDS, **kw)
    assert len(made) == 1 and made[0].n_streams == 3
    ts = made[0]
    assert pool1.log == pool0.log, "the decode pool sees the calls it saw"
    fast = {i for i, s in enumerate(SPEEDS) if s not in (None, 1.0)}
    # the resets: every request with a speed, once, with ITS speed, on the slot it took
    resets = [r for call in ts.resets for r in call]
    left = [s for _, s in resets]
    for i in fast:
        if min(LENS[i], 30) > 0:
            left.remove(SPEEDS[i])                                      # (ValueError: a request with audio took its slot without a reset)
    assert sorted(left) == sorted(SPEEDS[i] for i in fast if min(LENS[i], 30) == 0)[:len(left)], "nothing else but an empty request that held a slot"
    assert all(0 <= slot < 3 for slot, _ in resets)
    # one stretch call per decode call that holds a request with a speed, over exactly those slots and the PCM of that call
    decodes = [e for e in pool1.log if e[0] in ("decode", "decode_ragged")]
    with_pcm = [c for c in ts.calls if any(n for _, n, _ in c)]
    bare = [c for c in ts.calls if not any(n for _, n, _ in c)]
    assert 0 < len(with_pcm) <= len(decodes) and len(decodes) > 10
    k = 0
    for e in decodes:                                                   # in order: each stretch call is a sub-list of one decode call
        sizes = {i: 1920 * (e[2] if e[0] == "decode" else e[2][j]) for j, i in enumerate(e[1])}
        if k < len(with_pcm) and all(i in sizes and sizes[i] == n for i, n, _ in with_pcm[k]):
            k += 1
    assert k == len(with_pcm), "every stretch call takes the PCM of ONE decode call"
    assert all(f for c in bare for _, _, f in c), "an empty feed is only ever a closing one"
    for i in range(len(LENS)):
        a = [c for c in plain if c[0] == i]
        b = [c for c in got if c[0] == i]
        assert [c[3] for c in b] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        assert all(torch.equal(x[2], y[2]) for x, y in zip(a, b)), "the frames of every chunk are those of the plain run"
        assert torch.equal(torch.cat([c[1] for c in b]), torch.cat([c[1] for c in a])), f"request {i}: every sample once, the tail with the last chunk"
        if i not in fast:
            assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b)), "a request without a speed is not touched"
        elif min(LENS[i], 30) > 0:
            assert sum(c[1].numel() for c in b[:-1]) == sum(c[1].numel() for c in a[:-1]) - (LOOK if len(b) > 1 else 0), "held back until the close"
    closing = [[c for c in got if c[0] == i][-1] for i in fast if min(LENS[i], 30) > 0]
    assert any(c[2].shape[0] == 0 and c[1].numel() == LOOK for c in closing), "some request closes with a chunk that holds the tail alone"
    finals = sum(f for c in ts.calls for _, _, f in c)
    assert finals == len(resets), "final exactly once per stretched request that held a slot"


def test_the_stretch_runs_in_front_of_the_resampler(monkeypatch):
    plain, _, _, _ = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3)
    got, pool, made, made_rs = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3, speed=SPEEDS, out_sample_rate=48000)
    ts, rs = made[0], made_rs[0]
    # every resampler call that carries a stretched slot's samples follows that slot's stretch call, and gets what the stretch gave
    last_stretch = {}
    for kind, call in EVENTS:
        for i, n, f in call:
            if kind == "stretch":
                last_stretch[i] = (n, f)
            elif i in last_stretch and last_stretch[i] is not None:
                assert f == last_stretch[i][1], "final travels with the same chunk through both"
                last_stretch[i] = None
    assert [k for k, _ in EVENTS].count("resample") == len(rs.calls) and len(ts.calls) > 5
    for i in range(len(LENS)):                                          # both delays paid back by the close: every sample once
        a = torch.cat([c[1] for c in plain if c[0] == i])
        b = torch.cat([c[1] for c in got if c[0] == i])
        assert torch.equal(a, b)
    bare_rs = [c for c in rs.calls if all(f for _, _, f in c) and any(n == LOOK for _, n, _ in c)]
    assert bare_rs, "a closing chunk that is empty at 24 kHz hands the stretch's tail to the resampler"


def test_a_bad_speed_raises_before_anything_runs(monkeypatch):
    for bad in (0.4, 2.5, [1.2] * 3):
        with pytest.raises(ValueError, match="speed"):
            _run(_ScriptedSlots, LENS, 30, monkeypatch, speed=bad)


class _Gen(Gen):
    def generate_segments(self, prompts, *a, speed="absent", **kw):
        self.speeds = getattr(self, "speeds", []) + [speed]
        return super().generate_segments(prompts, *a, **kw)


def test_say_and_export_wav_hand_the_speed_on(tmp_path, monkeypatch):
    from sesameai import stretch as ts_mod
    calls = []
    monkeypatch.setattr(ts_mod, "stretch", lambda wavs, speed, **k: calls.append((len(wavs), speed)) or [w[::2] for w in wavs])
    gen = _Gen()
    tts = _tts(gen)
    tts.say(TEXT, output_filename=None, batch=3, speed=1.2)
    tts.say(TEXT, output_filename=None, batch=3)
    tts.export_wav(TEXT, str(tmp_path / "a.wav"), batch=2, speed=0.8)
    assert gen.speeds == [1.2, "absent", 0.8] and calls == [], "the batched path: generate_segments gets the speed, or is called as before"
    lens = []
    tts.say("One. Two words!", output_filename=None, on_segment=lambda pcm, sr: lens.append(len(pcm)), speed=2.0,
            start_silence_duration=500, end_silence_duration=100)
    assert calls == [(1, 2.0), (1, 2.0)], "the unbatched path: one device stretch per sentence, before the NumPy finish"
    assert lens == [5 * 1920 // 2 + 12000 + 2400] * 2, "lead and tail silence keep their lengths"
    tts.say("One.", output_filename=None, on_segment=lambda pcm, sr: lens.append(len(pcm)))
    tts.say("One.", output_filename=None, on_segment=lambda pcm, sr: lens.append(len(pcm)), speed=1.0)
    assert len(calls) == 2 and lens[-2:] == [5 * 1920 + 14400] * 2, "None and 1.0: no call at all"
    tts.export_wav("One.", str(tmp_path / "b.wav"), speed=1.5)
    assert calls[-1] == (1, 1.5)
    with pytest.raises(ValueError, match="speed"):
        tts.generate_audio_segment("One.", speed=3.0)


def test_the_cli_parses_speed(capsys):
    mod = _module()
    assert mod.parse_args(["hello"]).speed is None
    assert mod.parse_args(["hello", "--speed", "1.2"]).speed == 1.2
    assert mod.parse_args(["--speed", "0.5", "--batch", "4", "hello"]).speed == 0.5
    for bad in ("0.49", "2.01", "fast"):
        with pytest.raises(SystemExit):
            mod.parse_args(["hello", "--speed", bad])
    assert "--speed" in capsys.readouterr().err
