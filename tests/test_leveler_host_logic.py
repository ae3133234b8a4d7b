"""Host logic around the live leveler (no GPU): SlotStreams (sesameai/live_batch.py, through Generator.generate_many_stream) against
recording fake pools.  The fake leveler multiplies by a per-stream factor and holds nothing back, as the real one; what is checked is the
bookkeeping: ``loudness=None`` makes today's calls and imports nothing; a slot is reset with its request's ``Level``; ONE ``level_feed``
per pool call, after the stretch and before the mark and the resampler, ``final`` travelling with the same chunk; a None request never
touches the pool; an ending with nothing left to decode still gets its ``final``, with the stretch's tail; and ``Level``'s checked
conversion against tests/leveler_ref.py."""
import importlib
import sys

import pytest
import torch

import leveler_ref as R
from test_first_chunk_host_logic import _Codec
from test_host_logic import _ScriptedSlots, _ScriptedSlotsBeside
from test_resample_host_logic import _FakeResampler
from test_streams_host_logic import _scripts
from test_stretch_host_logic import LOOK, _FakeStretcher
from test_watermark_host_logic import KEY, _FakeMarker

EVENTS = []                          # ("stretch" | "level" | "mark" | "resample", the call) in the order the fakes were called


class _FakeLeveler:
    def __init__(self, n=3, device="cpu"):
        self.n_streams, self.calls, self.resets = n, [], []
        self._gain = [None] * n

    def level_reset(self, ids, levels):
        ids = [int(i) for i in ids]
        assert len(ids) == len(levels) >= 1
        self.resets.append(list(zip(ids, levels)))
        for i, lv in zip(ids, levels):
            self._gain[i] = float(lv.start_gain) * 0.5

    def level_feed(self, ids, chunks, final=False):
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, bool) else [bool(f) for f in final]
        assert len(set(ids)) == len(ids) == len(chunks) == len(fin) >= 1 and all(0 <= i < self.n_streams for i in ids)
        assert all(self._gain[i] is not None for i in ids), "a stream is fed only after its level_reset"
        self.calls.append([(i, int(c.shape[0]), f) for i, c, f in zip(ids, chunks, fin)])
        EVENTS.append(("level", self.calls[-1]))
        out = []
        for i, c, f in zip(ids, chunks, fin):
            assert c.dim() == 1 and c.dtype == torch.float32
            out.append(c.cpu() * self._gain[i])
            if f:
                self._gain[i] = None
        return out


def _logged(base, kind):
    class Logged(base):
        def feed(self, ids, chunks, final=False, **kw):
            out = super().feed(ids, chunks, final)
            EVENTS.append((kind, self.calls[-1]))
            return out
    return Logged


def _run(model_cls, lens, limit, monkeypatch, **kw):
    from sesameai import resample as rs_mod
    from sesameai import stretch as ts_mod
    from sesameai import watermarking as wm_mod
    from sesameai.generator import Generator
    made = {"level": [], "stretch": [], "mark": [], "resample": []}

    def maker(kind, cls):
        return lambda *a, **k: made[kind].append(cls(*a, **k)) or made[kind][-1]
    if kw.get("loudness") is not None:
        ld_mod = importlib.import_module("sesameai.loudness")             # (the one ``from .loudness import`` will find)
        monkeypatch.setattr(ld_mod, "LoudnessPool", maker("level", _FakeLeveler))
    monkeypatch.setattr(wm_mod, "WatermarkPool", maker("mark", _FakeMarker))              # (its own feed logs "mark" into ITS module's list)
    monkeypatch.setattr(ts_mod, "TimeStretchPool", maker("stretch", _logged(_FakeStretcher, "stretch")))
    monkeypatch.setattr(rs_mod, "ResamplerPool", maker("resample", _logged(_FakeResampler, "resample")))
    del EVENTS[:]
    codec = _Codec([])
    gen = Generator(model_cls(_scripts(lens, 11), 3), audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    texts = list(range(len(lens)))
    chunks = list(gen.generate_many_stream(texts, [0] * len(lens), [[]] * len(lens), max_audio_length_ms=limit * 80, **kw))
    return chunks, codec.pools[0], made


LENS = [3, 17, 0, 5, 40, 11, 20, 1, 22, 10, 33]
SPEEDS = [1.2, None, 0.8, 1.2, 2.0, None, 0.5, 1.0, 1.2, 1.5, 0.73]


def _levels():
    from sesameai.loudness import Level
    return [Level(-19.0), None, -23.0, Level(-16.0, start_gain=0.5), -19, None, Level(-19.0, slew_shift=2), -30.0, None, -19.0, Level(-14.0, ceiling_db=-3.0)]


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_no_loudness_makes_todays_calls_and_imports_nothing(model_cls, monkeypatch):
    plain, pool0, made0 = _run(model_cls, LENS, 30, monkeypatch)
    import sesameai
    if hasattr(sesameai, "loudness"):                                   # put back, afterwards, the module the other tests hold
        monkeypatch.setattr(sesameai, "loudness", sesameai.loudness)
    monkeypatch.delitem(sys.modules, "sesameai.loudness", raising=False)
    got, pool1, made = _run(model_cls, LENS, 30, monkeypatch, loudness=None)
    assert "sesameai.loudness" not in sys.modules, "loudness=None imports nothing"
    assert made["level"] == [] and EVENTS == []
    assert pool1.log == pool0.log and len(got) == len(plain)
    assert all(a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(plain, got))
    got, pool2, made = _run(model_cls, LENS, 30, monkeypatch, loudness=[None] * len(LENS))
    assert made["level"] == [] and EVENTS == [] and pool2.log == pool0.log, "nobody asks: no pool is built"


@pytest.mark.parametrize("first", [None, 3])
@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_slot_streams_level_every_decode_call_once_and_a_none_request_skips_the_pool(model_cls, first, monkeypatch):
    from sesameai.loudness import Level
    kw = {} if first is None else {"first_chunk_frames": first}
    levels = _levels()
    plain, pool0, _ = _run(model_cls, LENS, 30, monkeypatch, **kw)
    got, pool1, made = _run(model_cls, LENS, 30, monkeypatch, loudness=levels, **kw)
    assert len(made["level"]) == 1 and made["level"][0].n_streams == 3 and made["stretch"] == [] and made["mark"] == []
    lv = made["level"][0]
    assert pool1.log == pool0.log, "the decode pool sees the calls it saw"
    want = [None if v is None else v if isinstance(v, Level) else Level(float(v)) for v in levels]
    # the resets: every levelled request that held a slot, once, with ITS Level
    resets = [r for call in lv.resets for r in call]
    left = [l for _, l in resets]
    for i, l in enumerate(want):
        if l is not None and min(LENS[i], 30) > 0:
            left.remove(l)                                              # (ValueError: a request with audio took its slot without a reset)
    assert all(0 <= slot < 3 and isinstance(l, Level) for slot, l in resets) and len(left) <= 1
    # one level_feed per decode call that holds a levelled request, over exactly those slots and the PCM of that call
    decodes = [e for e in pool1.log if e[0] in ("decode", "decode_ragged")]
    with_pcm = [c for c in lv.calls if any(n for _, n, _ in c)]
    assert 0 < len(with_pcm) <= len(decodes) and len(decodes) > 10
    k = 0
    for e in decodes:
        sizes = {i: 1920 * (e[2] if e[0] == "decode" else e[2][j]) for j, i in enumerate(e[1])}
        if k < len(with_pcm) and all(i in sizes and sizes[i] == n for i, n, _ in with_pcm[k]):
            k += 1
    assert k == len(with_pcm), "every leveler call takes the PCM of ONE decode call"
    assert all(f for c in lv.calls if not any(n for _, n, _ in c) for _, _, f in c), "an empty feed is only ever a closing one"
    assert sum(f for c in lv.calls for _, _, f in c) == len(resets), "final exactly once per levelled request that held a slot"
    for i in range(len(LENS)):
        a = [c for c in plain if c[0] == i]
        b = [c for c in got if c[0] == i]
        assert [c[3] for c in b] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        assert all(torch.equal(x[2], y[2]) and x[1].shape == y[1].shape for x, y in zip(a, b)), "frames and lengths are the plain run's: nothing is held back"
        if want[i] is None:
            assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b)), "a request without a level is not touched"
        else:
            assert all(torch.equal(x[1] * (want[i].start_gain * 0.5), y[1]) for x, y in zip(a, b)), f"request {i} went through ITS stream"


def test_the_order_is_stretch_level_mark_resample_and_a_bare_ending_gets_its_final(monkeypatch):
    import test_watermark_host_logic as W
    monkeypatch.setattr(W, "EVENTS", EVENTS)                                # the fake marker logs where the others do
    levels = _levels()
    plain, _, _ = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3)
    got, pool, made = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3, speed=SPEEDS, out_sample_rate=48000, watermark=KEY,
                           loudness=levels)
    lv, ts, wm, rs = made["level"][0], made["stretch"][0], made["mark"][0], made["resample"][0]
    assert len(lv.calls) > 5 and len(ts.calls) > 5 and len(wm.calls) > 5 and len(rs.calls) > 5
    order = {"stretch": 0, "level": 1, "mark": 2, "resample": 3}
    per_slot = {}
    for kind, call in EVENTS:
        for i, n, f in call:
            per_slot.setdefault(i, []).append((kind, n, f))
    assert sorted(per_slot) == [0, 1, 2]
    shapes = set()
    for i, seq in per_slot.items():
        at = 0
        while at < len(seq):                                            # a pool call's group: ascending stages up to the resampler
            end = at
            while seq[end][0] != "resample":
                end += 1
            group = seq[at:end + 1]
            kinds = [k for k, _, _ in group]
            assert kinds == sorted(set(kinds), key=order.get) and kinds[-2:] == ["mark", "resample"], (i, group)
            assert len({f for _, _, f in group}) == 1, "final travels with the same chunk through every stage"
            if "level" in kinds:
                n_level = group[kinds.index("level")][1]
                if "stretch" in kinds and group[0][1] == 0:
                    assert group[0][2] and n_level == LOOK, "a bare ending: the leveler gets the stretch's tail, with final"
                    shapes.add("bare")
            shapes.add(tuple(kinds))
            at = end + 1
    assert ("stretch", "level", "mark", "resample") in shapes and ("level", "mark", "resample") in shapes and "bare" in shapes
    assert ("mark", "resample") in shapes and ("stretch", "mark", "resample") in shapes, "requests without a level skip the pool"
    # a bare ending WITHOUT a stretch still gets its final: an empty closing feed
    got2, _, made2 = _run(_ScriptedSlots, LENS, 30, monkeypatch, loudness=-19.0)
    lv2 = made2["level"][0]
    bare = [c for c in lv2.calls if not any(n for _, n, _ in c)]
    assert bare and all(f for c in bare for _, _, f in c)
    assert sum(f for c in lv2.calls for _, _, f in c) == sum(len(c) for c in lv2.resets)


def test_level_converts_to_the_rules_integers_and_refuses_the_rest():
    from sesameai.loudness import Level, per_request_levels
    assert Level(-19.0).params() == tuple(R.params(-19.0)) == (15848927, 29203, 65536, 16 * 65536, 4)
    for kw in (dict(ceiling_db=-3.0), dict(start_gain=0.5), dict(max_gain_db=12.0), dict(slew_shift=1), dict(slew_shift=16), dict(max_gain_db=36.0, start_gain=64.0)):
        assert Level(-23.0, **kw).params() == tuple(R.params(-23.0, **kw))
    for bad in (dict(max_gain_db=36.1), dict(max_gain_db=-97.0), dict(start_gain=0.0), dict(start_gain=16.1), dict(slew_shift=0), dict(slew_shift=17),
                dict(slew_shift=2.5), dict(ceiling_db=0.5)):
        with pytest.raises(ValueError):
            Level(-19.0, **bad).params()
    for bad in (1.0, -70.5):
        with pytest.raises(ValueError):
            Level(bad).params()
    assert per_request_levels(None, 2) == [None, None] and per_request_levels(-19, 2) == [Level(-19.0)] * 2
    assert per_request_levels([Level(-16.0, start_gain=0.5), None, -23], 3) == [Level(-16.0, start_gain=0.5), None, Level(-23.0)]
    with pytest.raises(ValueError):
        per_request_levels([-19, -20], 3)
    with pytest.raises(ValueError):
        per_request_levels([-19, 5.0], 2)
