"""Host logic of per-request sampling in the live batch (no GPU): scripted models stand in for the frame loop (tests/test_host_logic.py,
tests/test_prefix_host_logic.py) and record ``set_slot_sampling`` / ``clear_slot_sampling``.  What is checked is the scheduler's side of the
contract (sesameai/live_batch.py, both refill policies): a prompt with values of its own gets ONE set call for its slot immediately before
its refill call (after the prefix copy, if there is one), a slot such a prompt leaves is cleared before a prompt without own values takes
it, per-request values pass through generate_many / generate_many_stream, bad values raise before the model is touched -- and with
scalars and no seeds the model sees neither call."""
import pytest
import torch

from test_host_logic import _FakeCodec
from test_prefix_host_logic import VOICE_A, VOICE_B, _Beside, _prompts, _rows, _scripts, _Slots
from test_streams_host_logic import _FakeStreamCodec


class _Sampling:
    def set_slot_sampling(self, slots, temperature, topk, seed=None):
        self.log.append(("set", list(slots), temperature, topk, seed))

    def clear_slot_sampling(self, slots=None):
        self.log.append(("clear", None if slots is None else list(slots)))


class _SlotsS(_Sampling, _Slots):
    pass


class _BesideS(_Sampling, _Beside):
    pass


REFILLS = ("refill_slot", "refill_begin")
LENS = [3, 9, 4, 5, 14, 2, 7, 6, 3, 11, 8]


def _generator(model_cls, lens=LENS, seed=4):
    from sesameai.generator import Generator
    scripts = _scripts(lens, seed)
    model = model_cls(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=3)
    gen.refill_row_layers = 12
    return gen, model, scripts


def _check_order(log, own, with_prefix):
    """Every refill of a prompt with own values: log[k - 1] is its one set call, log[k - 2] the prefix copy where one belongs to it; a prompt
    without own values has no set in front of it, and a clear exactly when the slot's previous occupant had an entry."""
    holder = {}                                             # slot -> whether its current occupant has an entry
    n_set = 0
    for k, e in enumerate(log):
        if e[0] not in REFILLS:
            continue
        slot, i, kw = e[1], e[2], e[4]
        before = log[k - 1] if k else None
        if own[i] is not None:
            T, kk, seed = own[i]
            assert before == ("set", [slot], T, kk, seed), f"request {i}: {before} in front of its refill"
            n_set += 1
            if with_prefix and kw:
                first_step = next((j for j, x in enumerate(log) if x[0] == "step"), len(log))
                if k > first_step:                          # inside the live batch: copy, set, refill (the initial fill shares its copies up front)
                    assert log[k - 2][0] == "apply" and log[k - 2][2] == [slot], f"request {i}: {log[k - 2]}"
            holder[slot] = True
        else:
            if holder.get(slot):
                assert before == ("clear", [slot]), f"request {i} took slot {slot} from a prompt with an entry: {before}"
            else:
                assert before is None or before[0] not in ("set", "clear"), f"request {i}: {before}"
            holder[slot] = False
    assert n_set == sum(o is not None for o in own) == sum(e[0] == "set" for e in log)
    return holder


@pytest.mark.parametrize("with_prefix", [False, True])
@pytest.mark.parametrize("model_cls", [_SlotsS, _BesideS])
def test_set_sits_immediately_in_front_of_the_refill_and_a_reused_slot_is_cleared(model_cls, with_prefix):
    gen, model, scripts = _generator(model_cls)
    if with_prefix:
        gen.cache_prefix(*_rows(VOICE_A))
        gen.cache_prefix(*_rows(VOICE_B))
    del model.log[:]
    prompts, match = _prompts(len(LENS))
    # scalar (T, k); requests 0, 1, 4, 5, 8, 9 have a seed of their own: the others have no own values, so slots change hands both ways
    seeds = [1000 + i if i % 4 < 2 else None for i in range(len(LENS))]
    out = gen.generate_codes_continuous(prompts, 12, 0.9, 50, seed=seeds)
    for i, n in enumerate(LENS):
        assert torch.equal(out[i], scripts[i][: min(n, 12)].to(torch.int32)), f"request {i}"
    own = [(0.9, 50, s) if s is not None else None for s in seeds]
    _check_order(model.log, own, with_prefix)
    assert any(e[0] == "clear" for e in model.log), "no slot passed from a seeded request to a plain one: the case is not covered"
    assert all(e[1] is not None for e in model.log if e[0] == "clear")
    steps = [e for e in model.log if e[0] == "step"]
    assert steps and len([e for e in model.log if e[0] in REFILLS]) == len(LENS)
    if with_prefix:
        assert any(e[0] == "apply" for e in model.log) and [e[4] for e in model.log if e[0] in REFILLS and e[2] == 0] == [{"start": match[0]}]


@pytest.mark.parametrize("model_cls", [_SlotsS, _BesideS])
def test_sequences_give_every_prompt_an_entry_and_the_first_prompts_scalars_to_the_steps(model_cls):
    gen, model, _ = _generator(model_cls)
    prompts, _ = _prompts(len(LENS))
    temps = [0.9 if i % 2 == 0 else 0.8 for i in range(len(LENS))]
    ks = [50 if i % 2 == 0 else 40 for i in range(len(LENS))]
    seen = []
    step = model.step
    model.step = lambda B, T, k, use_graph=True: (seen.append((T, k)), step(B, T, k, use_graph))[1]
    gen.generate_codes_continuous(prompts, 12, temps, ks)
    own = [(temps[i], ks[i], None) for i in range(len(LENS))]
    _check_order(model.log, own, False)
    assert not any(e[0] == "clear" for e in model.log)
    assert seen and set(seen) == {(0.9, 50)}
    # one of the two as a sequence is enough; the seed rides along
    del model.log[:]
    gen.generate_codes_continuous(prompts[:4], 12, 0.7, [30, 31, 32, 33], seed=[None, 5, None, 1 << 40])
    _check_order(model.log, [(0.7, 30, None), (0.7, 31, 5), (0.7, 32, None), (0.7, 33, 1 << 40)], False)


@pytest.mark.parametrize("model_cls", [_SlotsS, _BesideS])
def test_scalars_and_no_seeds_make_neither_call(model_cls):
    gen, model, _ = _generator(model_cls)
    prompts, _ = _prompts(len(LENS))
    gen.generate_codes_continuous(prompts, 12, 0.9, 50)
    gen.generate_codes_continuous(prompts, 12, 0.9, 50, seed=[None] * len(LENS))
    assert not [e for e in model.log if e[0] in ("set", "clear")]
    assert len([e for e in model.log if e[0] in REFILLS]) == 2 * len(LENS)


@pytest.mark.parametrize("model_cls", [_SlotsS, _BesideS])
def test_generate_many_and_generate_many_stream_pass_the_requests_values_through(model_cls):
    from sesameai.generator import Generator
    lens = [3, 9, 4, 5, 7]
    scripts = _scripts(lens, 6)
    model = model_cls(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeStreamCodec(), max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    texts, n = list(range(len(lens))), len(lens)
    temps, ks, seeds = [0.9, 0.8, 0.9, 0.8, 0.7], [50, 40, 50, 40, 30], [11, None, 13, None, 15]
    own = list(zip(temps, ks, seeds))
    audio = gen.generate_many(texts, [0] * n, [[]] * n, max_audio_length_ms=12 * 80, temperature=temps, topk=ks, seed=seeds)
    assert [a.shape[0] for a in audio] == [1920 * x for x in lens]
    _check_order(model.log, own, False)
    del model.log[:]
    chunks = list(gen.generate_many_stream(texts, [0] * n, [[]] * n, max_audio_length_ms=12 * 80, temperature=temps, topk=ks, seed=seeds))
    assert sorted(i for i, _, _, last in chunks if last) == texts
    _check_order(model.log, own, False)


class _Untouchable:
    """Any use of the model is a failure: validation comes first."""
    _max_batch = 3
    device = torch.device("cpu")

    def setup_caches(self, b): pass

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were validated")


@pytest.mark.parametrize("kw", [
    dict(temperature=[0.9, 0.8], topk=50),                      # wrong lengths
    dict(temperature=0.9, topk=[50, 40, 30, 20]),
    dict(temperature=0.9, topk=50, seed=[1, 2]),
    dict(temperature=0.0, topk=50),                             # bad values
    dict(temperature=[0.9, -1.0, 0.9], topk=50),
    dict(temperature=float("nan"), topk=50),
    dict(temperature=0.9, topk=0),
    dict(temperature=0.9, topk=[50, 0, 50]),
])
def test_bad_values_raise_before_the_first_model_call(kw):
    from sesameai.generator import Generator
    gen = Generator(_Untouchable(), audio_tokenizer=_FakeCodec(), max_batch_size=3)
    prompts, _ = _prompts(3)
    args = dict(temperature=kw["temperature"], topk=kw["topk"])
    with pytest.raises(ValueError):
        gen.generate_codes_continuous(prompts, 12, args["temperature"], args["topk"], seed=kw.get("seed"))
    with pytest.raises(ValueError):
        list(gen._iter_blocks_continuous(prompts, 12, args["temperature"], args["topk"], None, seed=kw.get("seed")))
