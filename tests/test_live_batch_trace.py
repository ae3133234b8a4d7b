"""Trace equality of the continuously refilled batch (no GPU): the scripted models of tests/test_host_logic.py, with the logging wrappers
of tests/test_prefix_host_logic.py, are driven through ``Generator._iter_blocks_continuous`` and ``Generator.generate_many_stream``, and
every model call and everything yielded, in order, must equal what tests/golden/live_batch_traces.json holds.  The fixture was recorded
with this very recorder on the commit BEFORE the two hand-written loops became one scheduler (sesameai/live_batch.py); it is the pin that
host-side restructuring keeps the model calls (hence the Philox keys of every sampled frame) and the yields where they were.  Re-record it
(``python tests/test_live_batch_trace.py --record``) only on a commit whose behaviour is the intended reference, never to make a failure go.

Integer codes of a trace:
  calls   [0, slot, prompt, rows, start or -1] refill_slot   [1, slot, prompt, rows, start or -1] refill_begin   [2, k] refill_advance
          [3, prefix, slots...] apply_prefix   [4] step   [5, slots...] reset_slots   [6, first, n] read_frames
          [7, ids...] pool.reset   [8, T, ids...] pool.decode          (streams only)
  yields  -1 for the ``None`` tick, else the block's events [prompt, slot, frames, last, first code of each frame...];
          streams: one chunk [request, samples, frames, last, first code of each frame...]"""
import json
import os
import sys

import pytest

if __name__ == "__main__":                                               # (under pytest tests/conftest.py has set the import paths)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "sesameai-tts_amd")]

from test_host_logic import _FakeCodec
from test_prefix_host_logic import VOICE_A, VOICE_B, _Beside, _prompts, _rows, _scripts, _Slots
from test_streams_host_logic import _FakePool

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_batch_traces.json")

# utterance lengths (frames before the all-zero EOS frame): 0 = frame 0 is EOS; 8 / 9 / 10 / 11 / 16 end on poll boundaries of 8 and 10
# (frame 0 comes with the refill on the stalling path and out of the first step beside the loop); 40 runs into the limit
LENS = [8, 9, 0, 5, 40, 11, 10, 1, 22, 3, 16]
ONE_LIMIT = 25
PER_PROMPT = [25, 25, 25, 0, 25, 1, 25, 25, 10, 25, 8]
OPS = {"refill_slot": 0, "refill_begin": 1, "advance": 2, "apply": 3, "step": 4, "reset_slots": 5, "read_frames": 6}


class _MoreCalls:
    def reset_slots(self, slots):
        self.log.append(("reset_slots", *[int(s) for s in slots]))
        super().reset_slots(slots)

    def read_frames(self, B, first=0, n=None):
        self.log.append(("read_frames", int(first), int(n)))
        return super().read_frames(B, first, n)


class _LoggedSlots(_MoreCalls, _Slots):
    pass


class _LoggedBeside(_MoreCalls, _Beside):
    pass


KINDS = {"stalling": _LoggedSlots, "beside": _LoggedBeside}


def _encode(log):
    out = []
    for e in log:
        if isinstance(e[0], int):
            out.append(list(e))                                          # a pool call, already in numbers
        elif e[0] in ("refill_slot", "refill_begin"):
            assert set(e[4]) <= {"start"}
            out.append([OPS[e[0]], e[1], e[2], e[3], int(e[4].get("start", -1))])
        elif e[0] == "apply":
            out.append([OPS["apply"], e[1], *e[2]])
        else:
            out.append([OPS[e[0]], *e[1:]])
    return out


def _generator(kind, batch, prefixes, budget, n_prompts, codec=None):
    from sesameai.generator import Generator
    model = KINDS[kind](_scripts(LENS[:n_prompts], 21), batch)
    gen = Generator(model, audio_tokenizer=codec or _FakeCodec(), max_batch_size=batch)
    gen.refill_row_layers = budget
    for voice in ([], [VOICE_A, VOICE_B], [VOICE_A])[prefixes]:
        gen.cache_prefix(*_rows(voice))
    del model.log[:]
    return gen, model


def _limits(per_prompt, n_prompts):
    return PER_PROMPT[:n_prompts] if per_prompt else ONE_LIMIT


def record_blocks(kind, batch, poll, per_prompt, prefixes, budget, n_prompts=len(LENS)):
    gen, model = _generator(kind, batch, prefixes, budget, n_prompts)
    prompts, _ = _prompts(n_prompts)
    yields = []
    for block in gen._iter_blocks_continuous(prompts, _limits(per_prompt, n_prompts), 0.9, 50, poll):
        yields.append(-1 if block is None else
                      [[int(i), int(slot), int(fr.shape[0]), int(last), *fr[:, 0].tolist()] for i, slot, fr, last in block])
    return {"calls": _encode(model.log), "yields": yields}


class _LoggedPool(_FakePool):
    def __init__(self, n, max_chunk_frames, log):
        super().__init__(n, max_chunk_frames)
        self.log = log

    def reset(self, ids=None):
        self.log.append((7, *[int(i) for i in ids]))
        super().reset(ids)

    def decode(self, ids, codes):
        self.log.append((8, int(codes.shape[2]), *[int(i) for i in ids]))
        return super().decode(ids, codes)


class _LoggedStreamCodec(_FakeCodec):
    log = None

    def open_streams(self, n, max_chunk_frames=10):
        return _LoggedPool(n, max_chunk_frames, self.log)


def record_stream(kind, batch, per_prompt, prefixes, budget, n_prompts=len(LENS)):
    codec = _LoggedStreamCodec()
    gen, model = _generator(kind, batch, prefixes, budget, n_prompts, codec)
    codec.log = model.log                                                # pool calls in line with the model's: what is decoded beside which steps
    prompts, _ = _prompts(n_prompts)
    gen._text_ids = lambda text, speaker: prompts[int(text)][0][:, 32].tolist()
    limits = _limits(per_prompt, n_prompts)
    ms = [x * 80 for x in limits] if per_prompt else limits * 80
    chunks = []
    for i, pcm, fr, last in gen.generate_many_stream(list(range(n_prompts)), [0] * n_prompts, [[]] * n_prompts, max_audio_length_ms=ms):
        chunks.append([int(i), int(pcm.shape[0]), int(fr.shape[0]), int(last), *fr[:, 0].tolist()])
    return {"calls": _encode(model.log), "yields": chunks}


def _scenarios():
    """name -> (recorder, arguments).  Both model kinds x batch 1, 2, 3 x poll 1, 8, 10 x one limit / one per prompt (with a 0 and a 1), the
    prefix set (0 none, 1 two voices sharing a head -- request 8's match is capped at S - 1 --, 2 one voice) and the refill budget going
    round with them; every prefix set x budget once more at batch 3; more slots than prompts; the same through generate_many_stream."""
    out = {}
    budgets = (12, 20, 600)
    k = 0
    for kind in KINDS:
        for batch in (1, 2, 3):
            for poll in (1, 8, 10):
                for per_prompt in (0, 1):
                    out[f"blocks-{kind}-b{batch}-p{poll}-l{per_prompt}-x{k % 3}-r{budgets[k // 3 % 3]}"] = (
                        record_blocks, (kind, batch, poll, per_prompt, k % 3, budgets[k // 3 % 3]))
                    k += 1
        for prefixes in (0, 1, 2):
            for budget in budgets:
                out[f"blocks-{kind}-b3-p8-l1-x{prefixes}-r{budget}-again"] = (record_blocks, (kind, 3, 8, 1, prefixes, budget))
        for n_prompts in (1, 2):
            out[f"blocks-{kind}-b3-p8-l0-x1-r20-n{n_prompts}"] = (record_blocks, (kind, 3, 8, 0, 1, 20, n_prompts))
        for batch in (1, 2, 3):
            for per_prompt in (0, 1):
                for prefixes in (0, 1):
                    out[f"stream-{kind}-b{batch}-l{per_prompt}-x{prefixes}-r{budgets[k % 3]}"] = (
                        record_stream, (kind, batch, per_prompt, prefixes, budgets[k % 3]))
                    k += 1
        out[f"stream-{kind}-b3-l0-x1-r20-n2"] = (record_stream, (kind, 3, 0, 1, 20, 2))
    return out


SCENARIOS = _scenarios()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_scenarios(recorded):
    assert sorted(recorded) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_model_calls_and_yields_equal_the_recorded_trace(name, recorded):
    fn, args = SCENARIOS[name]
    got, want = fn(*args), recorded[name]
    for what in ("calls", "yields"):
        if got[what] != want[what]:
            k = next((k for k, (a, b) in enumerate(zip(got[what], want[what])) if a != b), min(len(got[what]), len(want[what])))
            pytest.fail(f"{name}: {what} differ from entry {k} on ({len(got[what])} against {len(want[what])} recorded): "
                        f"got {got[what][k:k + 4]}, recorded {want[what][k:k + 4]}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    with open(FIXTURE, "w") as f:
        json.dump({name: fn(*args) for name, (fn, args) in sorted(SCENARIOS.items())}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(SCENARIOS)} traces -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
