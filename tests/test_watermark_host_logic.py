"""Host logic around the watermark pool (no GPU): SlotStreams (sesameai/live_batch.py, through Generator.generate_many_stream) against
recording fake pools, ``watermark=`` / ``--watermark`` of the TTS service, and ``verify``'s decision rule on hand-made detect rows.  The
fake marker holds a stream's open block back like the real one and changes no sample, so a request's samples come out once and in order;
what is checked is the bookkeeping: today's calls when no watermark is asked for, ONE feed per decode call behind the stretch and in front
of the resampler, ``final`` on a request's last chunk, and a reset with the key when a request takes a slot."""
import pytest
import torch

from test_first_chunk_host_logic import _Codec
from test_host_logic import _ScriptedSlots, _ScriptedSlotsBeside
from test_resample_host_logic import _FakeResampler
from test_say_batch_host_logic import Gen, TEXT, _module, _tts
from test_streams_host_logic import _scripts
from test_stretch_host_logic import _FakeStretcher

S = 1920
KEY = [212, 211, 146, 56, 201]
EVENTS = []                          # ("stretch" | "mark" | "resample", the call) in the order the fakes were called


class _FakeMarker:
    def __init__(self, n=3, secret=None, device="cpu"):
        self.n_streams, self.secret, self.calls, self.resets = n, secret, [], []
        self._held = [torch.empty(0) for _ in range(n)]

    def reset(self, ids, payloads=None, t_q4=8):
        ids = [int(i) for i in ids]
        assert len(ids) == len(payloads) >= 1 and all(len(p) == 5 for p in payloads)
        self.resets.append([(i, list(p)) for i, p in zip(ids, payloads)])
        for i in ids:
            self._held[i] = torch.empty(0)

    def feed(self, ids, chunks, final=False):
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, bool) else [bool(f) for f in final]
        assert len(set(ids)) == len(ids) == len(chunks) == len(fin) >= 1 and all(0 <= i < self.n_streams for i in ids)
        self.calls.append([(i, int(c.shape[0]), f) for i, c, f in zip(ids, chunks, fin)])
        EVENTS.append(("mark", self.calls[-1]))
        out = []
        for i, c, f in zip(ids, chunks, fin):
            assert c.dim() == 1 and c.dtype == torch.float32
            x = torch.cat([self._held[i], c.cpu()])
            keep = 0 if f else x.shape[0] % S
            out.append(x[:x.shape[0] - keep])
            self._held[i] = x[x.shape[0] - keep:]
        return out


class _LoggedStretcher(_FakeStretcher):
    def feed(self, ids, chunks, final=False, want_offsets=False):
        out = super().feed(ids, chunks, final)
        EVENTS.append(("stretch", self.calls[-1]))
        return out


class _LoggedResampler(_FakeResampler):
    def feed(self, ids, chunks, final=False):
        out = super().feed(ids, chunks, final)
        EVENTS.append(("resample", self.calls[-1]))
        return out


def _run(model_cls, lens, limit, monkeypatch, **kw):
    from sesameai import resample as rs_mod
    from sesameai import stretch as ts_mod
    from sesameai import watermarking as wm_mod
    from sesameai.generator import Generator
    made, made_ts, made_rs = [], [], []
    monkeypatch.setattr(wm_mod, "WatermarkPool", lambda *a, **k: made.append(_FakeMarker(*a, **k)) or made[-1])
    monkeypatch.setattr(ts_mod, "TimeStretchPool", lambda *a, **k: made_ts.append(_LoggedStretcher(*a, **k)) or made_ts[-1])
    monkeypatch.setattr(rs_mod, "ResamplerPool", lambda *a, **k: made_rs.append(_LoggedResampler(*a, **k)) or made_rs[-1])
    del EVENTS[:]
    codec = _Codec([])
    gen = Generator(model_cls(_scripts(lens, 11), 3), audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    texts = list(range(len(lens)))
    chunks = list(gen.generate_many_stream(texts, [0] * len(lens), [[]] * len(lens), max_audio_length_ms=limit * 80, **kw))
    return chunks, codec.pools[0], made, made_ts, made_rs


LENS = [3, 17, 0, 5, 40, 11, 20, 1, 22, 10, 33]


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_no_watermark_builds_no_pool_and_makes_todays_calls(model_cls, monkeypatch):
    plain, pool0, made0, _, _ = _run(model_cls, LENS, 30, monkeypatch)
    got, pool1, made, _, _ = _run(model_cls, LENS, 30, monkeypatch, watermark=None)
    assert made0 == [] and made == [] and EVENTS == [], "no watermark: no pool is built"
    assert pool1.log == pool0.log and len(got) == len(plain)
    assert all(a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(plain, got))


@pytest.mark.parametrize("first", [None, 3])
@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_slot_streams_mark_every_decode_call_once(model_cls, first, monkeypatch):
    kw = {} if first is None else {"first_chunk_frames": first}
    plain, pool0, _, _, _ = _run(model_cls, LENS, 30, monkeypatch, **kw)
    got, pool1, made, made_ts, _ = _run(model_cls, LENS, 30, monkeypatch, watermark=True, **kw)
    assert len(made) == 1 and made[0].n_streams == 3 and made_ts == []
    assert made[0].secret == int.from_bytes(bytes(KEY), "big"), "the pool is keyed with the key's own 40-bit value"
    wm = made[0]
    assert pool1.log == pool0.log, "the decode pool sees the calls it saw"
    # a slot is reset, with the key, when a request takes it: once per request that held a slot
    resets = [r for call in wm.resets for r in call]
    assert all(0 <= slot < 3 and key == KEY for slot, key in resets)
    assert len(resets) >= sum(1 for n in LENS if min(n, 30) > 0)
    # one feed per decode call, over exactly that call's slots and PCM
    decodes = [e for e in pool1.log if e[0] in ("decode", "decode_ragged")]
    with_pcm = [c for c in wm.calls if any(n for _, n, _ in c)]
    assert len(with_pcm) == len(decodes) > 10
    for e, c in zip(decodes, with_pcm):
        sizes = [(i, S * (e[2] if e[0] == "decode" else e[2][j])) for j, i in enumerate(e[1])]
        assert [(i, n) for i, n, _ in c] == sizes, "ONE feed per pool call, the slots and the PCM of that call"
    assert all(f for c in wm.calls if not any(n for _, n, _ in c) for _, _, f in c), "an empty feed is only ever a closing one"
    assert sum(f for c in wm.calls for _, _, f in c) == len(resets), "final exactly once per request that held a slot"
    for i in range(len(LENS)):
        a = [c for c in plain if c[0] == i]
        b = [c for c in got if c[0] == i]
        assert [c[3] for c in b] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        # whole frames are whole blocks: nothing is held back, every chunk has the plain run's length and samples
        assert all(torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) for x, y in zip(a, b)), f"request {i}"


def test_the_mark_runs_behind_the_stretch_and_in_front_of_the_resampler(monkeypatch):
    speeds = [1.2, None, 0.8, 1.2, 2.0, None, 0.5, 1.0, 1.2, 1.5, 0.73]
    plain, _, _, _, _ = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3)
    got, pool, made, made_ts, made_rs = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3, speed=speeds, out_sample_rate=48000,
                                             watermark=KEY)
    wm, ts, rs = made[0], made_ts[0], made_rs[0]
    assert len(wm.calls) > 5 and len(ts.calls) > 5 and len(rs.calls) > 5
    # per slot every pool call is the group [stretch,] mark, resample -- in that order, and final travels with the same chunk through all
    per_slot = {}
    for kind, call in EVENTS:
        for i, n, f in call:
            per_slot.setdefault(i, []).append((kind, n, f))
    assert sorted(per_slot) == [0, 1, 2]
    for i, seq in per_slot.items():
        at = 0
        while at < len(seq):
            group = seq[at:at + 3] if seq[at][0] == "stretch" else seq[at:at + 2]
            assert [k for k, _, _ in group] == (["stretch", "mark", "resample"] if len(group) == 3 else ["mark", "resample"]), (i, seq[at:at + 4])
            assert len({f for _, _, f in group}) == 1, "final travels with the same chunk"
            if len(group) == 2:
                assert group[0][1] % S == 0, "without a stretch the mark gets whole frames"
            at += len(group)
    assert any(k == "stretch" for seq in per_slot.values() for k, _, _ in seq)
    for i in range(len(LENS)):                                          # all delays paid back by the close: every sample once
        a = torch.cat([c[1] for c in plain if c[0] == i])
        b = torch.cat([c[1] for c in got if c[0] == i])
        assert torch.equal(a, b), f"request {i}"


def test_a_bad_key_raises_before_anything_runs(monkeypatch):
    for bad in ([1, 2, 3], [1, 2, 3, 4, 256], "silentcipher"):
        with pytest.raises(ValueError):
            _run(_ScriptedSlots, LENS, 30, monkeypatch, watermark=bad)


class _Gen(Gen):
    def generate_segments(self, prompts, *a, watermark="absent", **kw):
        self.marks = getattr(self, "marks", []) + [watermark]
        return super().generate_segments(prompts, *a, **kw)


def test_tts_with_the_device_mark_hands_the_key_on_and_drops_the_post_hook(monkeypatch, capsys):
    mod = _module()
    made = []
    monkeypatch.setattr(mod, "load_csm_1b", lambda *a, **k: _Gen())
    monkeypatch.setattr(mod, "load_watermarker", lambda device, kind=None: made.append(kind) or ("marker", kind))
    tts = mod.TTS(voice_dir="/nonexistent", watermark="device")
    tts.load_model()
    assert made == ["device"] and tts.watermarker == ("marker", "device")
    tts.cached_context_tokens, tts.cached_context_masks = [torch.full((7, 33), 9).long()], [torch.ones(7, 33).bool()]
    tts.say(TEXT, output_filename=None, batch=3)
    gen = tts.generator
    assert gen.marks == [KEY] and gen.segment_calls[0]["post"] is None, "the device mark replaces the host post hook"
    plain = _tts(_Gen())
    plain.say(TEXT, output_filename=None, batch=3)
    assert plain.generator.marks == ["absent"], "no watermark: generate_segments is called as before"
    with pytest.raises(ValueError, match="watermark"):
        mod.TTS(voice_dir="/nonexistent", watermark="silentcipher")
    capsys.readouterr()


def test_the_cli_parses_watermark(capsys):
    mod = _module()
    assert mod.parse_args(["hello"]).watermark is None
    assert mod.parse_args(["hello", "--watermark", "device"]).watermark == "device"
    with pytest.raises(SystemExit):
        mod.parse_args(["hello", "--watermark", "loud"])
    assert "--watermark" in capsys.readouterr().err


def test_defaults_do_what_they_did():
    from sesameai import watermarking as wm
    x = torch.arange(10, dtype=torch.float32)
    y, rate = wm.watermark(None, x, 24000, wm.CSM_1B_GH_WATERMARK)
    assert y is x and rate == 24000 and wm.verify(None, x, 24000, wm.CSM_1B_GH_WATERMARK) is False
    with pytest.raises(ValueError, match="kind"):
        wm.load_watermarker("cuda", kind="loud")


def test_verify_decides_on_covered_and_wrong_symbols(monkeypatch):
    from sesameai import watermarking as wm
    cases = ((56, 56, True), (49, 56, True), (48, 56, False), (16, 16, True), (14, 16, True), (13, 16, False), (15, 15, False), (0, 0, False),
             (27, 27, True), (24, 27, True), (23, 27, False))
    for score, covered, want in cases:
        assert wm.verify_row(score, covered) is want, (score, covered)
        row = wm.DetectRow([3, 1003, score, covered, covered, 0xD4D39238C9, 1, 0] + [0] * 56)
        assert row.found is want and row.offset == 1003 and row.payload == KEY and row.crc_ok
    seen = []

    class _Marker(wm.DeviceWatermarker):
        def detect(self, audio, sample_rate, key, search=None):
            seen.append((sample_rate, list(key), search))
            return wm.DetectRow([0, 0, 50, 56, 56, 0, 0, 0] + [0] * 56)
    m = _Marker("cpu")
    assert wm.verify(m, torch.zeros(4), 24000, KEY) is True and wm.verify(m, torch.zeros(4), 16000, KEY, search=(5, 9)) is True
    assert seen == [(24000, KEY, None), (16000, KEY, (5, 9))], "search= is handed on; None asks for the full period"
    assert wm.symbol_bits(KEY) & 0xFF == int("{:08b}".format(0xB2)[::-1], 2), "the sync byte, MSB first, in the word's low bits"
    assert wm.crc8(KEY) == 74 and wm.default_secret(KEY) == 0xD4D39238C9
