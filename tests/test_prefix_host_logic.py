"""Host logic of the prefix store (no GPU): scripted models stand in for the frame loop (tests/test_host_logic.py) and record the
prefix calls.  What is checked is the bookkeeping of Generator.cache_prefix / the live batch (sesameai/live_batch.py, both refill policies): which prefix a prompt is matched
with and how far, that the copy sits immediately in front of the refill it belongs to, that only the rows after it are handed to the
model (at ``start = P``), that the refill budget counts those rows, that the initial fill seeds slots that share a prefix with one
call -- and that without a registered prefix the model sees exactly the calls it saw before."""
import pytest
import torch

from test_host_logic import _FakeCodec, _ScriptedSlots, _ScriptedSlotsBeside


class _Handle:
    def __init__(self, rows):
        self.rows, self.bytes, self.alive = rows, rows * 64, True

    def destroy(self):
        self.alive = False


class _PrefixCalls:
    """The prefix surface of sesameai.models.Model on a scripted model.  A prompt is known by the text token of its LAST row."""

    def _init_prefix(self):
        self.log, self.captured = [], []

    def prefill_prompt(self, tokens, mask):
        self.log.append(("prefill_prompt", tokens.shape[1]))
        return tokens.shape[1]

    def capture_prefix(self, slot, rows):
        self.log.append(("capture", slot, rows))
        self.captured.append(_Handle(rows))
        return self.captured[-1]

    def apply_prefix(self, handle, slots, rows=None):
        assert handle.alive
        self.log.append(("apply", self.captured.index(handle), list(slots)))

    def step(self, B, T, k, use_graph=True):
        self.log.append(("step",))
        super().step(B, T, k, use_graph)


class _Slots(_PrefixCalls, _ScriptedSlots):
    def __init__(self, scripts, max_batch):
        super().__init__(scripts, max_batch)
        self._init_prefix()

    def refill_slot(self, slot, tokens, mask, T, k, **kw):
        self.log.append(("refill_slot", slot, int(tokens[-1, 32]), tokens.shape[0], dict(kw)))
        return super().refill_slot(slot, tokens[-1:], mask[-1:], T, k)


class _Beside(_PrefixCalls, _ScriptedSlotsBeside):
    def __init__(self, scripts, max_batch):
        super().__init__(scripts, max_batch)
        self._init_prefix()

    def refill_begin(self, slot, tokens, mask, **kw):
        self.log.append(("refill_begin", slot, int(tokens[-1, 32]), tokens.shape[0], dict(kw)))
        super().refill_begin(slot, tokens[-1:], mask[-1:])

    def refill_advance(self, k):
        self.log.append(("advance", k))
        return super().refill_advance(k)


def _scripts(lens, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        sc = torch.randint(8, 2048, (n + 1, 32), generator=g); sc[n] = 0
        out.append(sc)
    return out


def _rows(ids):
    t = torch.zeros(len(ids), 33, dtype=torch.long); t[:, 32] = torch.tensor(ids)
    m = torch.zeros(len(ids), 33, dtype=torch.bool); m[:, 32] = True
    return t, m


VOICE_A = [900 + i for i in range(20)]
VOICE_B = [900, 901, 902] + [800 + i for i in range(9)]          # shares its first three rows with voice A


def _prompts(n):
    """request i: voice A (even) / voice B (odd) + 3 rows of its own; the last row names the request.  Request 4 matches neither voice,
    request 6 leaves voice A after 7 rows, request 8 IS voice A's first 12 rows (the match is capped at S - 1)."""
    out, match = [], []
    for i in range(n):
        voice = VOICE_A if i % 2 == 0 else VOICE_B
        ids, p = voice + [500 + i, 600 + i, i], len(voice)
        if i == 4:
            ids, p = [700, 701, 702, i], 0
        if i == 6:
            ids, p = VOICE_A[:7] + [650, 651, i], 7
        if i == 8:
            ids, p = VOICE_A[:11] + [i], 11
        out.append(_rows(ids)); match.append(p)
    return out, match


@pytest.mark.parametrize("model_cls", [_Slots, _Beside])
def test_without_a_registered_prefix_the_model_sees_the_calls_it_saw_before(model_cls):
    from sesameai.generator import Generator
    lens = [3, 9, 0, 5, 14, 2, 7]
    scripts = _scripts(lens, 3)
    model = model_cls(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=3)
    gen.refill_row_layers = 40
    prompts, _ = _prompts(len(lens))
    out = gen.generate_codes_continuous(prompts, 12, 0.9, 50)
    for i, n in enumerate(lens):
        assert torch.equal(out[i], scripts[i][: min(n, 12)].to(torch.int32))
    assert gen.prefixes == []
    assert not [e for e in model.log if e[0] in ("apply", "capture", "prefill_prompt")]
    refills = [e for e in model.log if e[0] in ("refill_slot", "refill_begin")]
    assert len(refills) == len(lens)
    for e in refills:
        assert e[3] == prompts[e[2]][0].shape[0] and e[4] == {}, "whole prompts, and no `start` argument"


@pytest.mark.parametrize("model_cls", [_Slots, _Beside])
def test_longest_match_is_copied_right_before_the_refill_and_only_the_suffix_runs(model_cls):
    from sesameai.generator import Generator
    lens = [3, 9, 4, 5, 14, 2, 7, 6, 3, 11, 8]
    scripts = _scripts(lens, 4)
    model = model_cls(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=3)
    gen.refill_row_layers = 12
    ha = gen.cache_prefix(*_rows(VOICE_A))
    hb = gen.cache_prefix(*_rows(VOICE_B))
    assert model.log == [("prefill_prompt", 20), ("capture", 0, 20), ("prefill_prompt", 12), ("capture", 0, 12)]
    assert gen.prefixes == [ha, hb] and (ha.rows, hb.rows) == (20, 12)
    del model.log[:]
    prompts, match = _prompts(len(lens))
    out = gen.generate_codes_continuous(prompts, 12, 0.9, 50)
    for i, n in enumerate(lens):
        assert torch.equal(out[i], scripts[i][: min(n, 12)].to(torch.int32)), f"request {i}"
    log = model.log
    refills = [(k, e) for k, e in enumerate(log) if e[0] in ("refill_slot", "refill_begin")]
    assert sorted(e[2] for _, e in refills) == list(range(len(lens)))
    first_step = next(k for k, e in enumerate(log) if e[0] == "step")
    for k, (_, slot, i, rows, kw) in refills:
        S, P = prompts[i][0].shape[0], match[i]
        assert rows == S - P, f"request {i}: {rows} rows handed to the model, {S - P} lie after its match"
        if P == 0:
            assert kw == {}, f"request {i} matches no prefix: the call is today's"
            continue
        assert kw == {"start": P}
        want = 0 if i % 2 == 0 else 1                       # voice A's snapshot / voice B's
        if k > first_step:                                  # inside the live batch: the copy is the call right before the refill
            assert log[k - 1] == ("apply", want, [slot]), f"request {i}: {log[k - 1]}"
        else:                                               # the initial fill: seeded together (below), no frame step in between
            applies = [e for e in log[:k] if e[0] == "apply" and slot in e[2]]
            assert applies and applies[-1][1] == want and not [e for e in log[:k] if e[0] == "step"]
    # the initial fill: requests 0 and 2 share voice A -> ONE copy for slots 0 and 2, one for request 1's voice B
    head = [e for e in log[:first_step] if e[0] == "apply"]
    assert ("apply", 0, [0, 2]) in head and ("apply", 1, [1]) in head and len(head) == 2
    if model_cls is _Beside:
        # the refill budget counts the rows that run: request 5 (voice B + 3 rows: 3 suffix rows) gets budget // 3 layers per call, capped at
        # all 16 -- with its whole 15 rows the same budget would have given fewer
        k5 = next(k for k, e in refills if e[2] == 5)
        adv = next(e for e in log[k5 + 1:] if e[0] == "advance")
        assert adv[1] >= min(12 // 3, 16) and adv[1] > max(1, 12 * 3 // 15)
    gen.drop_prefix(ha)
    assert gen.prefixes == [hb] and not ha.alive
    del model.log[:]
    gen.generate_codes_continuous(prompts[:1], 12, 0.9, 50)
    e = next(e for e in model.log if e[0] in ("refill_slot", "refill_begin"))
    assert e[3] == 23 - 3 and e[4] == {"start": 3}, "voice A is gone: request 0 shares only three rows with voice B"
